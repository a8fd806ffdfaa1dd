"""flow.decode_graphs / flow.generate_graphs (gnf_adj_edges_count_f32, gnf_adj_edges_fill) on the MI355X.

What is asserted and why the bounds are what they are:
  * against the existing decoder the edge lists are EQUAL (the kernels repeat k_pred_adj's fp32 expression term for term),
    at thresholds on both ends and in the middle, with and without self loops, over graph sizes that sit on every boundary
    of the bitmap (1, 63, 64, 65 nodes: the 64-column word; 130: three words; 17, 65, 130: 16-row tile tails; an empty
    graph), more rows than the scan has lanes (340 > 256), D = 1 / 3 / 200 and one D past the LDS row tile;
  * against the float64 oracle nothing is excluded either: the inputs are clustered with a margin (checked on the oracle
    alone in test_decode_graphs_cpu.py) that puts every pair at P >= 0.999 or P <= 1e-12, far from any threshold used;
  * the flow over the decoded graph is held to the project's 1e-4 (test_parity_gpu.py) against oracle.f on that edge list."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_graphs_ref as R
import per_graph_ref as PG
from helpers import graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NODE = [1, 63, 64, 65, 130, 0, 17]
THRESHOLDS = (0.0, 0.1, 0.5, 0.9, 1.0)
KEYS = ("senders", "receivers", "rowptr", "n_edge")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _shell(n_node, z):
    return graph_from_arrays(n_node, np.zeros(len(n_node), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)


def _draw(seed, n_node, d, c=0.6):
    """c D^(-1/4) randn: z_i - z_j has variance 2 c^2 / sqrt(D) per feature, so E[d2 / sqrt(D)] = 2 c^2 (0.72 for c = 0.6)
    whatever D is, and both outcomes are common: P > 0.9 <=> d2 / sqrt(D) < 0.78.  (With D^(+1/4) the mean would be
    0.72 D - at D = 200 every P is 0 and no threshold could tell a right edge list from an empty one.)"""
    rng = np.random.default_rng(seed)
    return (c * d ** -0.25 * rng.standard_normal((int(np.sum(n_node)), d))).astype(np.float32)


def _got(res):
    g = res["graph"]
    out = {"senders": g.senders.cpu().numpy(), "receivers": g.receivers.cpu().numpy(), "n_edge": g.n_edge.cpu().numpy(),
           "rowptr": res["csr"].rowptr.cpu().numpy(), "total": int(res["total_edges"])}
    assert g.senders.dtype == g.receivers.dtype == g.n_edge.dtype == res["csr"].rowptr.dtype == torch.int32
    assert res["total_edges"].dtype == torch.int64 and res["total_edges"].dim() == 0
    return out


def _assert_same(got, want, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")
    assert got["total"] == want["total"], what


def _pred_blocks(g):
    from gnf_amd.flow import pred_adj
    return [b.cpu().numpy() for b in pred_adj(g)]


# ---- 1. bit-equality with the existing decoder ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 200])
def test_edges_equal_thresholded_pred_adj(d):
    from gnf_amd.flow import decode_graphs
    g = _shell(N_NODE, _draw(d, N_NODE, d))
    blocks = _pred_blocks(g)
    seen = {}
    for t in THRESHOLDS:
        for loops in (False, True):
            want = R.edges_from_blocks(blocks, t, loops)
            res = decode_graphs(g, threshold=t, self_loops=loops)
            _assert_same(_got(res), want, f"D={d} t={t} loops={loops}")
            assert res["graph"].nodes is g.nodes and res["graph"].n_node is g.n_node
            assert res["graph"].edges.shape == (want["total"],) and float(res["graph"].edges.abs().sum()) == 0.0
            assert res["graph"].globals.shape == (len(N_NODE),)
            seen[t, loops] = want["total"]
    pairs = sum(n * (n - 1) for n in N_NODE)
    assert seen[1.0, False] == 0 and seen[1.0, True] == sum(N_NODE) and seen[0.0, True] > seen[0.5, True] - 1
    assert 0.05 * pairs < seen[0.9, False] < 0.95 * pairs          # both outcomes are common where it matters
    # a launch bound above the largest graph changes the bitmap's width, not the result
    res = decode_graphs(g, threshold=0.5, max_nodes_per_graph=200)
    _assert_same(_got(res), R.edges_from_blocks(blocks, 0.5, False), "max_nodes_per_graph=200")
    with pytest.raises(ValueError):
        decode_graphs(g, n_node_host=N_NODE, max_nodes_per_graph=129)


def test_empty_batch_and_empty_graphs():
    from gnf_amd.flow import decode_graphs
    for n_node in ([], [0, 0]):
        g = _shell(n_node, np.zeros((0, 4), np.float32))
        got = _got(decode_graphs(g, self_loops=True))
        assert got["total"] == 0 and got["rowptr"].tolist() == [0] and got["senders"].shape == (0,)
        assert got["n_edge"].tolist() == [0] * len(n_node)


def test_rows_wider_than_the_lds_tile():
    """16 x 1100 floats > 64 KB: the rows are read from global memory (same order of additions)"""
    from gnf_amd.flow import decode_graphs
    n_node, d = [19, 6], 1100
    g = _shell(n_node, _draw(5, n_node, d, c=0.7071))           # E[d2 / sqrt(D)] = 1: P = 0.5 in the middle
    blocks = _pred_blocks(g)
    for loops in (False, True):
        want = R.edges_from_blocks(blocks, 0.5, loops)
        assert 0.05 * 372 < want["total"] - loops * 25 < 0.95 * 372    # 19 * 18 + 6 * 5 ordered pairs
        _assert_same(_got(decode_graphs(g, self_loops=loops)), want)


# ---- 2. float64 oracle, nothing excluded -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 200])
def test_clustered_inputs_give_the_cliques(d):
    from gnf_amd.flow import decode_graphs
    z, lab = R.clustered_embeddings(np.random.default_rng(d), N_NODE, d)
    g = _shell(N_NODE, z)
    with np.errstate(over="ignore"):
        oracle_blocks = O.pred_adj_blocks(z, N_NODE)
    for loops in (False, True):
        closed = R.edges_from_blocks(R.clique_blocks(N_NODE, lab), 0.5, loops)
        for t in (0.1, 0.5, 0.9):
            got = _got(decode_graphs(g, threshold=t, self_loops=loops))
            _assert_same(got, closed, f"closed form, t={t}")
            _assert_same(got, R.edges_from_blocks(oracle_blocks, t, loops), f"float64 oracle, t={t}")


# ---- 3. CSR ----------------------------------------------------------------------------------------------------------------
def test_csr_is_what_build_csr_makes_of_the_edge_list():
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs
    g = _shell(N_NODE, _draw(8, N_NODE, 3))
    for loops in (False, True):
        res = decode_graphs(g, self_loops=loops)
        assert G.csr_of(res["graph"]) is res["csr"] and G.csr_of(res["graph"], by_sender=True) is res["csr"]
        assert res["csr"].n_nodes == sum(N_NODE) and res["csr"].n_edges == int(res["total_edges"]) > 0
        for by_sender in (False, True):
            ref = G.build_csr_device(res["graph"], by_sender)
            assert torch.equal(ref.rowptr, res["csr"].rowptr)
            assert torch.equal(ref.col[:ref.n_edges], res["csr"].col)


# ---- 4. strides ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 200])
def test_column_window_of_a_wider_buffer(d):
    from gnf_amd.flow import decode_graphs
    z = _draw(9, N_NODE, d)
    wide = torch.full((z.shape[0], d + 5), float("nan"), device=DEV)
    wide[:, 3:3 + d] = torch.as_tensor(z).to(DEV)
    g = _shell(N_NODE, z)
    win = g.replace(nodes=wide[:, 3:3 + d])
    assert win.nodes.stride(0) == d + 5 and win.nodes.data_ptr() % 16 != 0
    for loops in (False, True):
        _assert_same(_got(decode_graphs(win, self_loops=loops)), _got(decode_graphs(g, self_loops=loops)))


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------
def test_an_undersized_edge_buffer_is_truncated_never_overrun():
    from gnf_amd import _abi
    from gnf_amd.flow import decode_graphs
    lib = _abi.lib()
    z = _draw(10, N_NODE, 3)
    g = _shell(N_NODE, z)
    exact = _got(decode_graphs(g))
    cap, guard, sent = exact["total"] // 2, 64, -0x2152
    assert cap > 1000
    b, n, mx = len(N_NODE), sum(N_NODE), max(N_NODE)
    zt, nn = torch.as_tensor(z).to(DEV), torch.as_tensor(np.asarray(N_NODE, np.int32)).to(DEV)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    n_edge = torch.empty(b, dtype=torch.int32, device=DEV)
    total = torch.empty(1, dtype=torch.int64, device=DEV)
    ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, mx)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    bufs = [torch.full((cap + 2 * guard,), sent, dtype=torch.int32, device=DEV) for _ in range(2)]
    st = _abi.stream_ptr(torch.device(DEV))
    _abi.check(lib.gnf_adj_edges_count_f32(_abi.ptr(zt), 3, 3, _abi.ptr(nn), b, n, mx, 0.5, 0, _abi.ptr(rowptr),
                                           _abi.ptr(n_edge), _abi.ptr(total), _abi.ptr(ws), ws_bytes, st), "count")
    _abi.check(lib.gnf_adj_edges_fill(b, n, mx, _abi.ptr(rowptr), cap, C.c_void_p(bufs[0].data_ptr() + 4 * guard),
                                      C.c_void_p(bufs[1].data_ptr() + 4 * guard), _abi.ptr(ws), ws_bytes, st), "fill")
    torch.cuda.synchronize()
    assert int(total) == exact["total"]                                 # the true total, not the truncated one
    np.testing.assert_array_equal(rowptr.cpu().numpy(), exact["rowptr"])
    np.testing.assert_array_equal(n_edge.cpu().numpy(), exact["n_edge"])
    for buf, key in zip(bufs, ("senders", "receivers")):
        h = buf.cpu().numpy()
        np.testing.assert_array_equal(h[guard:guard + cap], exact[key][:cap])
        assert (h[:guard] == sent).all() and (h[guard + cap:] == sent).all(), f"guard band of {key} changed"
    # the same through decode_graphs: edge_capacity entries, the first min(total, capacity) valid, no copy to the host
    res = decode_graphs(g, edge_capacity=cap, n_node_host=N_NODE)
    assert res["graph"].senders.shape == res["graph"].receivers.shape == res["graph"].edges.shape == (cap,)
    assert int(res["total_edges"]) == exact["total"]
    np.testing.assert_array_equal(res["graph"].senders.cpu().numpy(), exact["senders"][:cap])
    np.testing.assert_array_equal(res["graph"].receivers.cpu().numpy(), exact["receivers"][:cap])
    np.testing.assert_array_equal(res["graph"].n_edge.cpu().numpy(), exact["n_edge"])


# ---- 6. capture ------------------------------------------------------------------------------------------------------------
def test_capacity_mode_is_capturable_and_replays_on_new_embeddings():
    from gnf_amd.flow import decode_graphs
    z1, z2 = _draw(11, N_NODE, 3), _draw(12, N_NODE, 3)
    g = _shell(N_NODE, z1)
    n2 = sum(n * n for n in N_NODE)
    eager = {}
    for name, z in (("z1", z1), ("z2", z2)):
        g.nodes.copy_(torch.as_tensor(z))
        eager[name] = _got(decode_graphs(g, self_loops=True))     # (also the kernels' first launches, outside the capture)
    assert eager["z1"]["total"] != eager["z2"]["total"]
    g.nodes.copy_(torch.as_tensor(z1))
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):      # one stream, a linear chain of launches
        res = decode_graphs(g, self_loops=True, edge_capacity=n2, n_node_host=N_NODE)
    for name, z in (("z1", z1), ("z2", z2), ("z1", z1)):
        g.nodes.copy_(torch.as_tensor(z))
        cg.replay()
        torch.cuda.synchronize()
        got, want = _got(res), eager[name]
        t = want["total"]
        assert got["total"] == t, name
        np.testing.assert_array_equal(got["senders"][:t], want["senders"])
        np.testing.assert_array_equal(got["receivers"][:t], want["receivers"])
        np.testing.assert_array_equal(got["rowptr"], want["rowptr"])
        np.testing.assert_array_equal(got["n_edge"], want["n_edge"])


# ---- 7. closing the loop ---------------------------------------------------------------------------------------------------
def test_the_flow_runs_on_the_decoded_graph(monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs, log_prob_per_graph, log_prob_terms
    n_node = [5, 17, 1, 30, 0, 12]
    hp = dict(D=8, latent=16, K=2, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
    x = _draw(13, n_node, 8)
    res = decode_graphs(_shell(n_node, x), self_loops=True)
    graph = res["graph"]
    s, r = graph.senders.cpu().numpy(), graph.receivers.cpu().numpy()
    n = sum(n_node)
    assert n < len(s) < sum(k * k for k in n_node)                   # self loops and more, not the complete graphs
    p = O.make_grevnet_params(3, 4, 16, 2, 2, final_scale=0.5)
    net = make_product_grevnet(hp, p)

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR decode_graphs seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    out = log_prob_terms(net, graph)
    per = log_prob_per_graph(net, graph)
    torch.cuda.synchronize()
    ref = O.Fp64Dense(s, r, n, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu").log_prob(x, p, 2)
    np.testing.assert_allclose(out["z_graph"].nodes.cpu().numpy(), ref["z"], atol=1e-4, rtol=1e-4)
    assert abs(float(out["log_det_jacobian"]) - ref["log_det_jacobian"]) <= 1e-4 * n
    assert abs(float(out["log_prob_xs_per_node"]) - ref["log_prob_xs_per_node"]) <= 1e-4
    pref = PG.PerGraphDense(s, r, n, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu").per_graph_terms(
        x, p, 2, np.asarray(n_node))
    want = pref["log_prob_xs"] / np.maximum(np.asarray(n_node, np.float64), 1.0)
    np.testing.assert_allclose(per["log_prob_xs_per_node"].cpu().numpy(), want, atol=1e-4, rtol=0)
    assert abs(float(per["log_prob_xs"].sum()) - ref["log_prob_xs"]) <= 1e-4 * n


# ---- 8. generate_graphs ----------------------------------------------------------------------------------------------------
def test_generate_graphs_is_sample_then_decode(grid_small):
    from gnf_amd.flow import generate_graphs, sample
    nn, ne, s, r = O.batch_graphs(*grid_small, [6, 7])
    n0 = int(nn[0])
    nn3, ne3 = np.array([nn[0], 0, nn[1]]), np.array([ne[0], 0, ne[1]])      # an empty graph in the middle
    n = int(nn3.sum())
    hp = dict(D=8, latent=16, K=3, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
    net = make_product_grevnet(hp, O.make_grevnet_params(2, 4, 16, 3, 2, final_scale=0.5))
    shell = graph_from_arrays(nn3, ne3, s, r, np.zeros((n, 8), np.float32), DEV)
    out = generate_graphs(net, shell, generator=torch.Generator(device=DEV).manual_seed(1))
    ref = sample(net, shell, generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(out["sample"], ref["sample"]) and torch.equal(out["grevnet_top_nodes"], ref["grevnet_top_nodes"])
    assert torch.equal(out["sample_log_prob"], ref["sample_log_prob"])
    want = R.edges_from_blocks(_pred_blocks(ref["grevnet_top"]), 0.5, False)
    _assert_same(_got(out), want)
    assert out["graph"].nodes is out["grevnet_top"].nodes
    slp = ref["sample_log_prob"].cpu().numpy()
    means = np.array([slp[:n0].mean(), 0.0, slp[n0:].mean()])
    got = out["sample_log_prob_per_graph"].cpu().numpy()
    assert got.dtype == np.float64 and got[1] == 0.0
    np.testing.assert_allclose(got, means, rtol=1e-12, atol=0)
    loops = generate_graphs(net, shell, generator=torch.Generator(device=DEV).manual_seed(1), threshold=0.9, self_loops=True)
    _assert_same(_got(loops), R.edges_from_blocks(_pred_blocks(ref["grevnet_top"]), 0.9, True))
