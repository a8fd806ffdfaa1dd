"""Per-graph likelihood of generated graphs from the inverse pass (gnf_grevnet_inverse_per_graph_f32, GRevNet.g_per_graph,
flow.sample_per_graph, flow.generate_graphs(log_prob=True)) on the MI355X, against the float64 reference of
tests/inverse_per_graph_ref.py: every GNN family, every kernel the inverse walk can take (asserted by gnf_last_route), batch
norm with the moving statistics, row strides and guard bands, errors before any launch, empty cases, hipGraph capture.

Tolerances are those tests/test_per_graph_gpu.py applies to the forward terms: per node of EACH graph 1e-4 on the three sums,
3e-4 on x; blocks that end in LayerNorm: 1e-4 + 6 x the error of the CPU fp32 restatement on the same inputs.  The cases live
in tests/inverse_per_graph_cases.py; tests/test_inverse_per_graph_cpu.py checks on the CPU that their seeds leave the fp32
restatement inside half of these bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import inverse_per_graph_cases as IC
from helpers import GuardBanded, graph_from_arrays, make_product_grevnet
from per_graph_ref import single_graph_batches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _host_sums(gs):
    """sums[k] as a sequential fp64 host loop over graph_out[:, k]"""
    out = [0.0, 0.0]
    for row in gs.cpu().numpy():
        out[0] += float(row[0])
        out[1] += float(row[1])
    return out


def _check(net, nn, ne, s, r, z, ref, tol=IC.TOL, x_tol=IC.X_TOL):
    """parity per graph, x bitwise g's, reproducible, sums = the host loop, plain g / f unchanged by the call; returns the
    graph, the terms and the route of the per-graph call"""
    from gnf_amd import _abi
    from gnf_amd.flow import inverse_per_graph
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    x_before = net.g(graph).nodes.clone()
    zf_before, _ = net.f(graph)
    zf_before, fs_before = zf_before.nodes.clone(), net.last_sums.clone()
    out = inverse_per_graph(net, graph)
    route = _abi.last_route()
    gs, sums, x = net.last_graph_sums.clone(), net.last_sums.clone(), out["grevnet_top_nodes"].clone()
    torch.cuda.synchronize()
    err = IC.per_node_errors({k: out[k].cpu().numpy() for k in ("log_det_jacobian", "log_prob_zs", "log_prob_xs")}, ref, nn)
    for key, e in err.items():
        print(f"[inverse-per-graph] {key}: max per-node error over {len(nn)} graphs {e:.3e} (tol {tol:.1e})")
    for key, e in err.items():
        assert e <= tol, (key, e)
    np.testing.assert_allclose(out["log_prob_xs_per_node"].cpu().numpy(), ref["log_prob_xs_per_node"], atol=tol)
    np.testing.assert_array_equal(out["num_nodes"].cpu().numpy(), np.asarray(nn, np.float64))
    np.testing.assert_allclose(x.cpu().numpy(), ref["x"], atol=x_tol, rtol=x_tol)
    assert torch.equal(graph.nodes.cpu(), torch.as_tensor(np.asarray(z, np.float32)))   # the source rows are read only
    # bitwise: x is g's; two calls give the same bits; sums are the graph-order sums
    assert torch.equal(x, x_before)
    net.g_per_graph(graph)
    torch.cuda.synchronize()
    assert torch.equal(net.last_graph_sums, gs) and torch.equal(net.last_sums, sums)
    want = _host_sums(gs)
    assert float(sums[0]) == want[0] and float(sums[1]) == want[1], (sums.tolist(), want)
    # a plain g and a plain f after the call return what they returned before it
    assert torch.equal(net.g(graph).nodes, x_before)
    zf, _ = net.f(graph)
    assert torch.equal(zf.nodes, zf_before) and torch.equal(net.last_sums, fs_before)
    return graph, out, route


# ---- parity: every GNN family, fused and layered, with and without batch norm ---------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("case", IC.MP_CASES, ids=[f"D{c[0]}_L{c[1]}_{c[4]}_{c[5]}_{c[7]}" for c in IC.MP_CASES])
def test_message_passing_parity(case, bn, fused):
    hp, nn, ne, s, r, z, p = IC.mp_case(case, bn)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert "row_sums" in route and (fused or "layered" in route), route


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("shape", IC.ATTN_CASES + [IC.ATTN_DATA_DRIVER, IC.ATTN_FRONT_GENERIC],
                         ids=[f"D{s[0]}_h{s[4]}_kq{s[5]}" for s in IC.ATTN_CASES + [IC.ATTN_DATA_DRIVER, IC.ATTN_FRONT_GENERIC]])
def test_edge_attention_parity(shape, bn, fused):
    """both drivers' head geometries (8 x 10 / 10 / C 80; 1 x 64 / 64 / C 64 on complete graphs), a block without concat, and
    heads of 10 / 10 at H = 16.  Fused, the 10 / 10 geometries run the attention prologue of k_half_fused - with batch norm
    its bijector-on-load form - and must leave the row sums from there: the instance compiled for the default geometry
    (fused_fixed) and the any-geometry one"""
    hp, nn, ne, s, r, z, p = IC.attn_case(shape, bn, False)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert "row_sums" in route, route
    if fused and shape == IC.ATTN_CASES[0]:
        assert {"fused_front", "fused_fixed", "fused_16"} <= route and "attn_pair" not in route, route
    elif fused and shape == IC.ATTN_FRONT_GENERIC:
        assert {"fused_front", "fused_16"} <= route and not {"attn_pair", "fused_fixed"} & route, route
    else:   # (heads wider than 16, or the layered path: the front-end runs as launches of its own)
        assert "attn_pair" in route and "fused_front" not in route, route


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_edge_attention_residual_layer_norm_parity(fused):
    hp, nn, ne, s, r, z, p = IC.attn_case(IC.ATTN_RESIDUAL, False, True)
    ref = IC.dense_ref(hp, nn, s, r, z, p)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _, _, route = _check(net, nn, ne, s, r, z, ref, tol=IC.ln_tol(hp, nn, s, r, z, p, ref))
    assert {"row_sums", "layer_norm", "coupling"} <= route, route


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("kind", ["self_attn", "multihead"])
def test_graph_scope_attention_parity(kind, bn, fused):
    hp, nn, ne, s, r, z, p = IC.graph_attn_case(kind, bn)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _, _, route = _check(net, nn, ne, s, r, z, IC.gather_ref(hp, nn, s, r, z, p))
    assert "row_sums" in route and "attn_pair" in route, route


# ---- the smallest shapes that can go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_tile_and_graph_boundaries(fused):
    """ring + chord graphs of 1, 17, 16, 33 and 2 nodes (69 rows: N = 5 mod 16): a boundary inside a tile, a graph over three
    tiles, a one-node graph, an edgeless graph"""
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], True, batch=IC.edge_batch())
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_one_live_row_in_the_last_tile_and_an_empty_graph_between_two(fused):
    """N = 33 = 1 mod 16, graphs of 16, 0 and 17 nodes: the empty graph gets {0, 0} and 0 per node, not NaN"""
    batch = IC.ring_chord_batch([16, 0, 17], edgeless=())
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], True, batch=batch)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _, out, _ = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert float(net.last_graph_sums[1].abs().max()) == 0.0
    assert float(out["log_prob_xs"][1]) == 0.0 and float(out["log_prob_xs_per_node"][1]) == 0.0


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("h", [1, 3, 50])
def test_padded_coupling_widths(h, fused):
    hp, nn, ne, s, r, z, p = IC.width_case(h, True)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))


# ---- forced routes ---------------------------------------------------------------------------------------------------------
FORCED = {12: {"fused_16"}, 22: {"fused_32"}, 11: {"one_net_16", "coupling"}, 21: {"one_net_32", "coupling"},
          10: {"big"}, 20: {"big"}, 30: {"big"}, 40: {"big"}}


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("shape", sorted(FORCED))
def test_forced_shapes_message_passing(shape, bn):
    """the both-nets shapes (coupling in k_half_fused), one net per workgroup + k_coupling, and the large-batch kernel with
    1 .. 4 row tiles per workgroup at most, on a batch of 9 row tiles"""
    from gnf_amd import _abi
    batch = IC.dataset_batch("community_medium", [3, 77, 150, 9])
    hp, nn, ne, s, r, z, p = IC.mp_case((64, 256, 5, 2, "mean", "agg", False, "sparse"), bn, batch=batch)
    net = make_product_grevnet(hp, p)
    _abi.set_option("force_shape", shape)
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert FORCED[shape] | {"row_sums"} <= route and "layered" not in route and "fused_geo" not in route, route
    assert len(route & {"fused_16", "fused_32", "one_net_16", "one_net_32", "big", "big_split"}) == 1, route


def test_the_geometry_instance_is_replaced_by_the_generic_one_with_the_same_bits():
    """the bench's default MLP on a small batch: a plain g runs k_half_fused_geo, which has no per-row form; g_per_graph takes
    the generic 16-row instance instead and x must still be the plain call's bits (_check holds it to that)"""
    from gnf_amd import _abi
    batch = IC.dataset_batch("community_medium", [3, 77, 150, 9])
    hp, nn, ne, s, r, z, p = IC.mp_case((64, 256, 5, 2, "mean", "agg", False, "sparse"), False, batch=batch)
    net = make_product_grevnet(hp, p)
    graph, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert {"fused_16", "row_sums"} <= route and "fused_geo" not in route, route
    net.g(graph)
    assert _abi.last_route() == {"fused_geo"}


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("attn_kernel", [1, 2, 3])
def test_forced_attention_kernels(attn_kernel, bn):
    """the front-end kept out of the fused kernel's prologue: the MLP kernel reads h0 from memory, same epilogue"""
    from gnf_amd import _abi
    hp, nn, ne, s, r, z, p = IC.attn_case(IC.ATTN_CASES[0], bn, False)
    net = make_product_grevnet(hp, p)
    _abi.set_option("attn_kernel", attn_kernel)
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert {"attn_pair", "row_sums"} <= route and "fused_front" not in route, route


@pytest.mark.parametrize("shape", [22, 40])
def test_forced_shapes_edge_attention_residual(shape):
    """residual blocks add x_cond to s in the epilogue: the row sums must carry it (32-row shape, large-batch kernel)"""
    from gnf_amd import _abi
    hp, nn, ne, s, r, z, p = IC.attn_case(IC.ATTN_RESIDUAL, False, False)
    net = make_product_grevnet(hp, p)
    _abi.set_option("force_shape", shape)
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert ({"fused_32"} if shape == 22 else {"big"}) | {"row_sums"} <= route, route


def _bench_batch(workload, graphs):
    """bench.py's batch, weights and features of a workload with `graphs` graphs"""
    import bench
    saved = (bench.WORKLOAD, bench.GRAPHS_PER_GPU, dict(bench.HP))
    try:
        bench.WORKLOAD = bench.WORKLOADS[workload]
        bench.GRAPHS_PER_GPU = graphs
        bench.HP.update(bench.WORKLOAD["hp"])
        dicts, _, _ = bench.make_batch(1, 0)
        hp = dict(bench.HP)
        params = bench.make_params(bench.WEIGHT_SEED, hp, bench.FINAL_SCALE)
    finally:
        bench.WORKLOAD, bench.GRAPHS_PER_GPU = saved[0], saved[1]
        bench.HP.clear()
        bench.HP.update(saved[2])
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    return data_dicts_to_graphs_tuple(dicts), params, hp


def test_split_row_tiles_of_the_large_batch_kernel():
    """the config-4 batch of 53 graphs, whose even deal splits row tiles between two workgroups: the workgroup that couples a
    split tile writes its rows' sums.  x bitwise the 32-row shape's and the plain g's, the per-graph values up to the order
    of the row sums' additions (fp64: 1e-9 relative is generous)"""
    from gnf_amd import _abi
    g_cpu, p, hp = _bench_batch("config4", 53)
    nn = g_cpu.n_node.numpy()
    hp1 = dict(hp, T=1)
    p1 = {k: [[half[0]] for half in p[k]] for k in ("s", "t")}
    net = make_product_grevnet(hp1, p1)
    graph = graph_from_arrays(nn, g_cpu.n_edge.numpy(), g_cpu.senders.numpy(), g_cpu.receivers.numpy(), g_cpu.nodes.numpy(), DEV)
    res = {}
    for shape in (22, 40):
        _abi.set_option("force_shape", shape)
        xg, _ = net.g_per_graph(graph)
        route = _abi.last_route()
        res[shape] = (xg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone())
        assert torch.equal(net.g(graph).nodes, res[shape][0])
        if shape == 40:
            assert {"big_split", "row_sums"} <= route, route   # (this device's CU count gives the deal split tiles)
        else:
            assert {"fused_32", "row_sums"} <= route, route
    torch.cuda.synchronize()
    assert torch.equal(res[22][0], res[40][0])
    # the split path's numbers against the fp64 reference (gather formulation: the batch is too large for the dense one)
    ref = IC.gather_ref(dict(hp1, weight_sharing=False), nn, g_cpu.senders.numpy(), g_cpu.receivers.numpy(), g_cpu.nodes.numpy(), p1)
    d = g_cpu.nodes.shape[1]
    for shape in (22, 40):
        gs = res[shape][1].cpu().numpy()
        zs = -0.5 * gs[:, 1] - 0.5 * d * IC.IP.LN_2PI * nn
        err = IC.per_node_errors({"log_det_jacobian": gs[:, 0], "log_prob_zs": zs, "log_prob_xs": zs - gs[:, 0]}, ref, nn)
        print(f"[inverse-per-graph] config-4 batch of {int(nn.sum())} nodes, force_shape {shape}: per-node errors {err}")
        assert max(err.values()) <= IC.TOL, (shape, err)
    a, b = res[22][1].cpu().numpy(), res[40][1].cpu().numpy()
    assert np.isfinite(b).all()
    np.testing.assert_allclose(b, a, rtol=1e-9, atol=1e-9)
    want = _host_sums(res[40][1])
    assert float(res[40][2][0]) == want[0] and float(res[40][2][1]) == want[1]


def test_wide_nets_on_the_layered_path():
    """the data driver's 2048 x 3 nets at D = 200: too wide for the fused kernels - the wide-layer GEMMs, the last layer's
    partial-product slabs, k_coupling"""
    hp, nn, ne, s, r, z, p = IC.mp_case((200, 2048, 3, 2, "mean", "agg", False, "sparse"), True)
    net = make_product_grevnet(hp, p)
    _, _, route = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    assert {"layered", "coupling", "row_sums"} <= route, route


# ---- in place / out of place, layouts ---------------------------------------------------------------------------------------
def _raw_call(net, graph, src, ld_src, dst, ld, d, sums, gout, ws_ptr, ws_bytes):
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    flow = net._flow(d // 2, torch.device(DEV))
    csr = csr_desc(graph, csr_of(graph), True)
    with torch.cuda.device(DEV):
        return lib.gnf_grevnet_inverse_per_graph_f32(C.byref(csr), C.byref(flow), src, ld_src, dst, ld, d, C.c_void_p(sums.data_ptr()),
                                                     C.c_void_p(gout.data_ptr()), ws_ptr, ws_bytes, _abi.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
def test_in_place_equals_out_of_place_bit_for_bit(bn, fused):
    from gnf_amd import _abi
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], bn, batch=IC.edge_batch())
    net = make_product_grevnet(hp, p)
    net.fused = fused
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    xg, _ = net.g_per_graph(graph)
    want = (xg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone())
    n, d, b = z.shape[0], z.shape[1], len(nn)
    lib = _abi.lib()
    ws_bytes = lib.gnf_inverse_per_graph_workspace_bytes(n, b, d, C.byref(net._flow(d // 2, torch.device(DEV))))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    for src_null in (True, False):   # z_src NULL, z_src == x
        buf = graph.nodes.clone()
        sums = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
        gout = torch.full((b, 2), float("nan"), dtype=torch.float64, device=DEV)
        rc = _raw_call(net, graph, None if src_null else _abi.ptr(buf), d, _abi.ptr(buf), d, d, sums, gout, _abi.ptr(ws), ws_bytes)
        torch.cuda.synchronize()
        assert rc == 0, lib.gnf_last_error()
        assert torch.equal(buf, want[0]) and torch.equal(gout, want[1]) and torch.equal(sums, want[2])


@pytest.mark.parametrize("layout", [(72, 0, 96, 0), (67, 1, 81, 3), (64, 0, 64, 0)], ids=["padded", "misaligned", "dense"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_row_strides_and_guard_bands(layout, fused):
    """ld_src > D, a misaligned base, guard-banded source, destination, sums, graph_out and workspace: nothing outside
    graph_out[0 : 2 n_graphs], sums, x and the workspace is written, and the numbers are those of the contiguous call"""
    from gnf_amd import _abi
    lds_, c0s, ldd, c0d = layout
    batch = IC.dataset_batch("community_medium", [3, 77, 150, 9])
    hp, nn, ne, s, r, z, p = IC.mp_case((64, 256, 5, 2, "mean", "agg", False, "sparse"), False, batch=batch)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    xg, _ = net.g_per_graph(graph)
    want_x, want_gs, want_sums = xg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone()
    n, d, b = z.shape[0], 64, len(nn)
    lib = _abi.lib()
    src = GuardBanded(n, d, lds_, c0s, device=DEV, fill=z)
    dst = GuardBanded(n, d, ldd, c0d, device=DEV)
    ws_bytes = lib.gnf_inverse_per_graph_workspace_bytes(n, b, d, C.byref(net._flow(d // 2, torch.device(DEV))))
    outs = torch.full((2 + 2 * b + 64,), float("nan"), dtype=torch.float64, device=DEV)
    sums, gout = outs[16:18], outs[32:32 + 2 * b]
    ws_words = (ws_bytes + 7) // 8
    wsbuf = torch.full((ws_words + 2 * 512,), float("nan"), dtype=torch.float64, device=DEV)
    rc = _raw_call(net, graph, src.ptr(), lds_, dst.ptr(), ldd, d, sums, gout, C.c_void_p(wsbuf.data_ptr() + 512 * 8), ws_bytes)
    torch.cuda.synchronize()
    assert rc == 0, lib.gnf_last_error()
    src.check_guard(), dst.check_guard()
    np.testing.assert_array_equal(src.numpy(), z)                       # the source is read only
    assert torch.isnan(outs[:16]).all() and torch.isnan(outs[18:32]).all() and torch.isnan(outs[32 + 2 * b:]).all()
    assert torch.isnan(wsbuf[:512]).all() and torch.isnan(wsbuf[512 + ws_words:]).all()
    got_x = dst.window.clone()
    assert torch.equal(gout.view(b, 2)[:, 1], want_gs[:, 1])           # sum z^2 of the same source values, the same order
    if src.aligned() and dst.aligned():   # the same vector / scalar load decisions: the same bits
        assert torch.equal(got_x, want_x) and torch.equal(gout.view(b, 2), want_gs) and torch.equal(sums, want_sums)
    else:   # (other load widths may add a row's neighbours up in another order: the parity tests' tolerances)
        np.testing.assert_allclose(got_x.cpu().numpy(), want_x.cpu().numpy(), atol=IC.X_TOL, rtol=IC.X_TOL)
        err = (gout.view(b, 2) - want_gs).abs().cpu().numpy() / np.maximum(np.asarray(nn, np.float64), 1.0)[:, None]
        assert err[:, 0].max() <= IC.TOL, err.max(axis=0)


# ---- independence and the round trip ----------------------------------------------------------------------------------------
def test_with_batch_norm_a_graph_in_a_batch_equals_the_graph_alone():
    """the bijectors of g use constants: each graph's three values from the batched call agree with a single-graph call of
    the same flow within twice the per-node bound - the check the forward direction cannot offer"""
    from gnf_amd.flow import inverse_per_graph
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], True)
    net = make_product_grevnet(hp, p)
    _, out, _ = _check(net, nn, ne, s, r, z, IC.dense_ref(hp, nn, s, r, z, p))
    keys = ("log_det_jacobian", "log_prob_zs", "log_prob_xs")
    got = {k: out[k].cpu().numpy() for k in keys}
    for g, (n1, e1, s1, r1, z1) in enumerate(single_graph_batches(nn, ne, s, r, z)):
        alone = inverse_per_graph(net, graph_from_arrays(n1, e1, s1, r1, z1, DEV))
        for k in keys:
            assert abs(float(alone[k][0]) - got[k][g]) / max(int(nn[g]), 1) <= 2 * IC.TOL, (g, k)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_round_trip_f_per_graph_of_g_per_graph(fused):
    """without batch norm f inverts g: f_per_graph's per-graph log-det at g(z) is minus logdet_g, within the sum of the two
    sides' own bounds (2e-4 per node)"""
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], False)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    xg, logdet_g = net.g_per_graph(graph)
    logdet_g = logdet_g.clone()
    _, logdet_f = net.f_per_graph(xg)
    torch.cuda.synchronize()
    err = (logdet_f + logdet_g).abs().cpu().numpy() / np.maximum(np.asarray(nn, np.float64), 1.0)
    print(f"[inverse-per-graph] round trip: max per-node |logdet_f + logdet_g| {err.max():.3e}")
    assert err.max() <= 2e-4


# ---- errors before any launch, empty cases ------------------------------------------------------------------------------------
def test_errors_come_before_any_launch():
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_of
    hp, nn, ne, s, r, z, p = IC.mp_case((8, 16, 2, 1, "mean", "agg", False, "sparse"), True)
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    lib = _abi.lib()
    n, b = z.shape[0], len(nn)
    flow = net._flow(4, torch.device(DEV))
    ws_bytes = lib.gnf_inverse_per_graph_workspace_bytes(n, b, 8, C.byref(flow))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((n, 8), 7.0, device=DEV)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    gout = torch.full((b, 2), 7.0, dtype=torch.float64, device=DEV)
    st = _abi.stream_ptr(torch.device(DEV))
    fn = lib.gnf_grevnet_inverse_per_graph_f32

    def untouched():
        torch.cuda.synchronize()
        return all(float(t.min()) == 7.0 and float(t.max()) == 7.0 for t in (out, sums, gout))
    # missing node_offsets (the descriptor of a call that does not need them)
    rc = fn(C.byref(csr_of(graph).desc), C.byref(flow), _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, _abi.ptr(sums), _abi.ptr(gout),
            _abi.ptr(ws), ws_bytes, st)
    assert rc == -1 and "node_offsets" in lib.gnf_last_error().decode() and untouched()
    # null graph_out / sums, a short workspace
    assert _raw_call(net, graph, _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, sums, torch.empty(0), _abi.ptr(ws), ws_bytes) == -1 and untouched()
    assert _raw_call(net, graph, _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, torch.empty(0), gout, _abi.ptr(ws), ws_bytes) == -1 and untouched()
    assert _raw_call(net, graph, _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, sums, gout, _abi.ptr(ws), ws_bytes - 1) == -3 and untouched()
    # a bijector without moving statistics (validate_bn's inverse rule)
    saved = flow.bns[1].moving_variance
    flow.bns[1].moving_variance = None
    try:
        rc = _raw_call(net, graph, _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, sums, gout, _abi.ptr(ws), ws_bytes)
        assert rc == -1 and "moving" in lib.gnf_last_error().decode() and untouched()
    finally:
        flow.bns[1].moving_variance = saved
    assert _raw_call(net, graph, _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8, sums, gout, _abi.ptr(ws), ws_bytes) == 0
    torch.cuda.synchronize()
    assert float(out.min()) != 7.0 and torch.isfinite(gout).all()


def test_empty_batch_and_a_batch_of_only_empty_graphs():
    from gnf_amd.flow import sample_per_graph
    hp, nn, ne, s, r, z, p = IC.mp_case((8, 16, 2, 1, "mean", "agg", False, "sparse"), True)
    net = make_product_grevnet(hp, p)
    none = np.zeros(0, np.int32)
    for sizes in ([0, 0, 0], []):
        empty = graph_from_arrays(sizes, sizes, none, none, np.zeros((0, 8), np.float32), DEV)
        net.last_sums = None
        out = sample_per_graph(net, empty)
        torch.cuda.synchronize()
        for key in ("log_det_jacobian", "log_prob_zs", "log_prob_xs", "num_nodes", "log_prob_xs_per_node"):
            assert out[key].shape == (len(sizes),) and out[key].dtype == torch.float64
            assert len(sizes) == 0 or float(out[key].abs().max()) == 0.0
        assert out["grevnet_top_nodes"].shape == (0, 8) and float(net.last_sums.abs().max()) == 0.0


# ---- capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
def test_g_per_graph_captured_and_replayed_with_new_latent_values(bn):
    batch = IC.dataset_batch("community_medium", [3, 77, 150, 9, 20, 21])
    hp, nn, ne, s, r, z, p = IC.mp_case((64, 256, 5, 2, "mean", "agg", False, "sparse"), bn, batch=batch)
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, z, DEV)
    z1 = graph.nodes.clone()
    z2 = torch.as_tensor(np.random.default_rng(9).standard_normal(z.shape).astype(np.float32)).to(DEV)
    eager = {}
    for name, zv in (("z1", z1), ("z2", z2)):
        graph.nodes.copy_(zv)
        xg, _ = net.g_per_graph(graph)      # (also the first launches: caches, per-device kernel attributes)
        eager[name] = (xg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone())
    assert float((eager["z1"][1] - eager["z2"][1]).abs().max()) > 0
    graph.nodes.copy_(z1)
    torch.cuda.synchronize()
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        x_c, _ = net.g_per_graph(graph, sums)
        gs_c = net.last_graph_sums
    for name, zv in (("z2", z2), ("z1", z1), ("z2", z2)):
        graph.nodes.copy_(zv)
        x_c.nodes.zero_(), gs_c.zero_(), sums.zero_()
        cg.replay()
        torch.cuda.synchronize()
        x_e, gs_e, s_e = eager[name]
        assert torch.equal(x_c.nodes, x_e), name
        assert torch.equal(gs_c, gs_e), name
        assert torch.equal(sums, s_e), name


# ---- generate_graphs -----------------------------------------------------------------------------------------------------------
def test_generate_graphs_default_is_unchanged_and_log_prob_adds_the_five_tensors():
    from gnf_amd.flow import PER_GRAPH_KEYS, decode_graphs, generate_graphs, sample
    from gnf_amd.sharding import gather_per_graph
    hp, nn, ne, s, r, z, p = IC.mp_case(IC.MP_CASES[1], True)
    net = make_product_grevnet(hp, p)
    shell = graph_from_arrays(nn, ne, s, r, np.zeros_like(z), DEV)

    def gen(seed=31):
        return torch.Generator(device=DEV).manual_seed(seed)
    base = generate_graphs(net, shell, generator=gen())
    assert set(base) == {"graph", "csr", "total_edges", "sample", "sample_log_prob", "grevnet_top", "grevnet_top_nodes",
                         "sample_log_prob_per_graph"}
    smp = sample(net, shell, generator=gen())
    dec = decode_graphs(smp["grevnet_top"])
    assert torch.equal(base["sample"], smp["sample"]) and torch.equal(base["grevnet_top_nodes"], smp["grevnet_top_nodes"])
    assert torch.equal(base["sample_log_prob"], smp["sample_log_prob"])
    for key in ("senders", "receivers", "n_node", "n_edge"):
        assert torch.equal(getattr(base["graph"], key), getattr(dec["graph"], key)), key
    assert int(base["total_edges"]) == int(dec["total_edges"])
    full = generate_graphs(net, shell, generator=gen(), log_prob=True)
    assert set(full) == set(base) | set(PER_GRAPH_KEYS) and len(PER_GRAPH_KEYS) == 5
    for key in ("sample", "sample_log_prob", "grevnet_top_nodes", "sample_log_prob_per_graph"):
        assert torch.equal(full[key], base[key]), key
    for key in ("senders", "receivers", "n_node", "n_edge"):
        assert torch.equal(getattr(full["graph"], key), getattr(base["graph"], key)), key
    ref = IC.dense_ref(hp, nn, s, r, full["sample"].cpu().numpy(), p)
    err = IC.per_node_errors({k: full[k].cpu().numpy() for k in ("log_det_jacobian", "log_prob_zs", "log_prob_xs")}, ref, nn)
    assert max(err.values()) <= IC.TOL, err
    np.testing.assert_allclose(full["log_prob_xs_per_node"].cpu().numpy(), ref["log_prob_xs_per_node"], atol=IC.TOL)
    for key in PER_GRAPH_KEYS:   # one rank: the permutation alone
        assert full[key].shape == (len(nn),) and full[key].dtype == torch.float64 and full[key].device.type == "cuda"
        assert torch.equal(gather_per_graph(full[key], [np.arange(len(nn))]), full[key])
