"""gnf_amd.adj_loss.binary_loss (gnf_adj_loss_f32) on the MI355X against the float64 restatement of tests/adj_loss_ref.py.

Inputs: graphs of [1, 0, 17, 16, 33, 65, 2, 64] nodes (tile edge, bitmap word edge, an empty and a 1-node graph), embeddings of
the first seed in range(16) whose float64 logits keep 2 delta_ij from the kinks u = +-U and u = 0 (adj_loss_ref.pick_seed: a
condition on the inputs, test_adj_loss_cpu.py asserts such a seed exists for every batch used here).  No pair is left out of
any comparison.

Bounds.  loss_per_graph: sum over the graph's ordered pairs of delta_ij + 2^-20 (1 + ce_ij) - the logit's fp32 error through
|d ce / d u| <= 1, plus a few ulp of the fp32 softplus; sum_loss the sum of those, mean_loss that over N^2 - N.  The pair counts
are EQUAL (the margin makes them well defined).  grad_nodes: 1e-3 of max |reference gradient|, the yardstick of
test_train_gpu.py.  Widths: 1 and 2 (the smallest, a gradient row narrower than a wave), 7 (odd), 64 (config 2's), 200 (the
data driver's), 400 and 1030 - one per kernel instance: 64 columns per chunk in LDS up to D = 191, 32 up to 330, the row tile
alone up to 960, nothing in LDS beyond."""
import functools

import numpy as np
import pytest
import torch

import adj_loss_ref as R
from helpers import GuardBanded, graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("sum_loss", "mean_loss", "loss_per_graph", "false_positive_pairs", "false_negative_pairs")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


@functools.lru_cache(maxsize=None)
def _case(d, dist=R.SCALED_HACKY, soft=False, sizes=tuple(R.SIZES), dup=False, symmetric=False):
    """(z fp32, (n_edge, s, r), float64 reference) of the first seed with margin - computed once per case"""
    seed, z, graph = R.pick_seed(list(sizes), d, dist, duplicate_rows=dup, symmetric=symmetric)
    assert seed is not None, "no seed in range(16) satisfies the margin condition"
    return z, graph, R.binary_loss(z, list(sizes), graph[1], graph[2], dist, soft)


def _graphs(z, sizes, graph):
    """(embeddings GraphsTuple without edges, true GraphsTuple) on the device"""
    n_edge, s, r = graph
    none = np.zeros(0, np.int32)
    emb = graph_from_arrays(sizes, np.zeros(len(sizes), np.int32), none, none, z, DEV)
    true = graph_from_arrays(sizes, n_edge, s, r, np.zeros((len(z), 1), np.float32), DEV)
    return emb, true


def _token(dist):
    from gnf_amd import adj_loss
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    if dist == R.SCALED_HACKY:
        return scaled_hacky_sigmoid_l2
    return adj_loss.hacky_sigmoid_l2 if dist == R.HACKY else adj_loss.sigmoid_l2(dist[0], dist[1])


def _check(d, dist, soft, sizes, dup=False, symmetric=False):
    from gnf_amd.adj_loss import binary_loss
    z, graph, ref = _case(d, dist, soft, tuple(sizes), dup, symmetric)
    emb, true = _graphs(z, sizes, graph)
    n, b = len(z), len(sizes)
    fn = _token(dist)
    plain = binary_loss(emb, true, fn, soft)
    out = binary_loss(emb, true, fn, soft, grad="sum")
    mean = binary_loss(emb, true, fn, soft, grad="mean", n_node_host=sizes)
    assert set(plain) == set(KEYS) and set(out) == set(KEYS) | {"grad_nodes"}
    for k in KEYS:   # the gradient changes no other output, nor do the sizes given on the host
        assert torch.equal(plain[k], out[k]) and torch.equal(mean[k], out[k]), k
    assert out["sum_loss"].dtype == torch.float64 and out["sum_loss"].dim() == 0 and out["mean_loss"].dim() == 0
    assert out["loss_per_graph"].dtype == torch.float64 and out["loss_per_graph"].shape == (b,)
    assert out["false_positive_pairs"].dtype == torch.int64 and out["false_negative_pairs"].shape == (b,)
    assert out["grad_nodes"].dtype == torch.float32 and out["grad_nodes"].shape == (n, d)
    assert all(v.device.type == "cuda" for v in out.values())
    bound = R.loss_bounds(ref, d, dist)
    loss = out["loss_per_graph"].cpu().numpy()
    err = np.abs(loss - ref["loss_per_graph"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"D={d} {dist} soft={soft}: loss error over bound {worst:.3g} (largest |err| {err.max():.3g}), sum_loss "
          f"{float(out['sum_loss']):.17g} vs {ref['sum_loss']:.17g}")
    assert (err <= bound).all(), (err, bound)
    assert abs(float(out["sum_loss"]) - ref["sum_loss"]) <= bound.sum()
    assert abs(float(out["mean_loss"]) - ref["mean_loss"]) <= bound.sum() / (n * n - n)
    np.testing.assert_array_equal(out["false_positive_pairs"].cpu().numpy(), ref["fp"])
    np.testing.assert_array_equal(out["false_negative_pairs"].cpu().numpy(), ref["fn"])
    scale = np.abs(ref["grad"]).max()
    g_sum, g_mean = out["grad_nodes"].cpu().numpy(), mean["grad_nodes"].cpu().numpy()
    e_sum, e_mean = np.abs(g_sum - ref["grad"]).max(), np.abs(g_mean - ref["grad"] / (n * n - n)).max()
    print(f"  grad: |err| {e_sum:.3g} of max |g| {scale:.3g} (sum), {e_mean:.3g} of {scale / (n * n - n):.3g} (mean)")
    assert scale > 0.1 and e_sum <= 1e-3 * scale and e_mean <= 1e-3 * scale / (n * n - n)
    o = 0
    for g, ng in enumerate(sizes):   # the empty and the 1-node graph: zeros, and a 1-node graph's gradient row is exactly zero
        if ng < 2:
            assert loss[g] == 0.0 and int(out["false_positive_pairs"][g]) == 0 == int(out["false_negative_pairs"][g])
            assert not g_sum[o:o + ng].any() and not g_mean[o:o + ng].any()
        o += ng
    return out, ref


# ---- 1. parity with the float64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("d", [1, 2, 7, 64, 200, 400, 1030])
def test_parity_with_float64(d, soft):
    _check(d, R.SCALED_HACKY, soft, R.SIZES)


def test_parity_on_a_symmetric_graph_and_the_host_helpers():
    from gnf_amd import adj_loss
    out, ref = _check(7, R.SCALED_HACKY, False, R.SIZES, symmetric=True)
    assert (ref["fp"] % 2 == 0).all() and (ref["fn"] % 2 == 0).all()
    per_graph = adj_loss.incorrect_edges_per_graph(out)
    assert per_graph.dtype == torch.int32 and per_graph.tolist() == ((ref["fp"] + ref["fn"]) // 2).tolist()
    assert float(adj_loss.false_positive_edges(out)) == ref["fp"].sum() / 2.0
    assert float(adj_loss.false_negative_edges(out)) == ref["fn"].sum() / 2.0
    assert float(adj_loss.total_incorrect_edges(out)) == (ref["fp"].sum() + ref["fn"].sum()) / 2.0


# ---- 2. tied to the decoder: no margin needed ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 200])
def test_counts_equal_pred_adj_thresholded(d):
    from gnf_amd.adj_loss import binary_loss
    from gnf_amd.flow import pred_adj
    z = R.embeddings(R.SIZES, d, 5, duplicate_rows=True)
    graph = R.true_graph(R.SIZES, 5)
    emb, true = _graphs(z, R.SIZES, graph)
    out = binary_loss(emb, true)
    blocks = pred_adj(emb)
    labels = R.graph_blocks(z, R.SIZES, graph[1], graph[2])
    assert float(blocks[2][0, 1]) == float(blocks[2][2, 3]) > 0.99      # d2 = 0: sigmoid(10)
    fp, fn = [], []
    for p, lab in zip(blocks, labels):
        a = torch.as_tensor(lab["a"].astype(np.float32)).to(DEV)
        fp.append(int((p - a > 0.5).sum()))
        fn.append(int((a - p > 0.5).sum()))
    assert sum(fp) > 100 and sum(fn) > 100
    assert out["false_positive_pairs"].tolist() == fp and out["false_negative_pairs"].tolist() == fn


# ---- 3. round trip through decode_graphs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
def test_decoded_graph_scores_zero_against_its_own_embeddings(self_loops):
    from gnf_amd.adj_loss import binary_loss
    from gnf_amd.flow import decode_graphs, pred_adj
    z = R.embeddings(R.SIZES, 7, 2, duplicate_rows=True)
    emb, _ = _graphs(z, R.SIZES, R.true_graph(R.SIZES, 2))
    b = len(R.SIZES)
    own = decode_graphs(emb, threshold=0.5, self_loops=self_loops)["graph"]
    assert int(own.n_edge.sum()) > 1000
    out = binary_loss(emb, own)
    assert out["false_positive_pairs"].tolist() == [0] * b == out["false_negative_pairs"].tolist()
    assert float(out["sum_loss"]) > 0.0
    strict = decode_graphs(emb, threshold=0.9, self_loops=self_loops)["graph"]
    out = binary_loss(emb, strict)
    likely = torch.stack([(p > 0.5).sum() for p in pred_adj(emb)])       # (the blocks' diagonal is 0)
    edges = strict.n_edge.to(torch.int64) - (torch.as_tensor(R.SIZES).to(DEV) if self_loops else 0)
    assert out["false_negative_pairs"].tolist() == [0] * b
    assert out["false_positive_pairs"].tolist() == (likely - edges).tolist() and int((likely - edges).sum()) > 0


# ---- 4. the other distance functions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,dup", [(R.HACKY, False), (R.sigmoid_l2(3.0, 2.0), False), (R.sigmoid_l2(20.0, 1.0), True)],
                         ids=["hacky_sigmoid_l2", "sigmoid_l2(3,2)", "sigmoid_l2(20,1)"])
def test_other_distance_functions(dist, dup):
    _, ref = _check(7, dist, False, R.SIZES, dup=dup)
    if dup:   # two identical rows: u = 20 > U, the upper clip, c_ij = 0
        assert any((b["clipped"] & (b["u"] > R.U)).any() for b in ref["blocks"])


# ---- 5. more than one column chunk, five bitmap words ----------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_graph_of_300_nodes(soft):
    _check(16, R.SCALED_HACKY, soft, [300, 3])


# ---- 6. strided input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ld,c0", [(7, 13, 3), (64, 72, 4), (200, 203, 1)])
def test_strided_nodes_are_bit_equal(d, ld, c0):
    from gnf_amd.adj_loss import binary_loss
    z, graph, _ = _case(d)
    emb, true = _graphs(z, R.SIZES, graph)
    want = binary_loss(emb, true, grad="sum", use_soft_labels=True)
    gb = GuardBanded(len(z), d, ld, c0=c0, device=DEV, fill=z)
    assert gb.window.stride(0) == ld and gb.window.data_ptr() != gb.bits.data_ptr()
    got = binary_loss(emb.replace(nodes=gb.window), true, grad="sum", use_soft_labels=True)
    for k in KEYS + ("grad_nodes",):
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["grad_nodes"]).all())
    gb.check_guard()


def test_a_clipped_pair_adds_exactly_nothing_even_where_an_embedding_is_not_finite():
    """c_ij = 0 is skipped, not multiplied: a node at infinity (every pair with it clipped) and a 1-node graph at NaN leave
    every output as it is with the node merely far away, bit for bit, and their own gradient rows exactly zero"""
    from gnf_amd.adj_loss import binary_loss
    sizes = [1, 17, 40]
    z = R.embeddings(sizes, 7, 3)
    graph = R.true_graph(sizes, 3)
    far = z.copy()
    far[0], far[1 + 4], far[1 + 17 + 33] = 1e3, 1e3, -1e3
    wild = far.copy()
    wild[0], wild[1 + 4], wild[1 + 17 + 33] = np.nan, np.inf, -np.inf
    outs = []
    for zz in (far, wild):
        emb, true = _graphs(zz, sizes, graph)
        outs.append(binary_loss(emb, true, grad="sum", use_soft_labels=True))
    for k in KEYS + ("grad_nodes",):
        assert torch.equal(outs[0][k], outs[1][k]), k
    g = outs[1]["grad_nodes"]
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.1
    assert not g[0].any() and not g[1 + 4].any() and not g[1 + 17 + 33].any()
    assert float(outs[1]["loss_per_graph"][0]) == 0.0 and bool(torch.isfinite(outs[1]["loss_per_graph"]).all())


# ---- 7. bit-reproducible ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 200, 1030])
def test_two_calls_give_the_same_bits(d):
    from gnf_amd.adj_loss import binary_loss
    z, graph, _ = _case(d)
    emb, true = _graphs(z, R.SIZES, graph)
    first = binary_loss(emb, true, grad="mean")
    again = binary_loss(emb, true, grad="mean")
    for k in KEYS + ("grad_nodes",):
        assert torch.equal(first[k], again[k]), k


# ---- 8. capture ------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_new_embeddings():
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured on one stream,
    z is overwritten in place, and the replay equals an eager call on the new z bit for bit."""
    from gnf_amd.adj_loss import binary_loss
    z, graph, _ = _case(64)
    emb, true = _graphs(z, R.SIZES, graph)
    binary_loss(emb, true, grad="sum", max_nodes_per_graph=65)           # (the first launches: CSR and offsets caches)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = binary_loss(emb, true, grad="sum", max_nodes_per_graph=65)
    for seed in (11, 12, 13, 14):   # (a workspace zeroed by a memset node lost rows from the second replay on)
        emb.nodes.copy_(torch.as_tensor(R.embeddings(R.SIZES, 64, seed)).to(DEV))
        for v in captured.values():
            v.zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = binary_loss(emb, true, grad="sum", max_nodes_per_graph=65)
        for k in KEYS + ("grad_nodes",):
            assert torch.equal(captured[k], eager[k]), k
        assert float(eager["sum_loss"]) > 0.0


# ---- 9. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    from gnf_amd import _abi
    from gnf_amd.adj_loss import binary_loss
    z, graph, _ = _case(7)
    emb, true = _graphs(z, R.SIZES, graph)
    with pytest.raises(_abi.GnfError):
        binary_loss(emb.to("cpu"), true)
    with pytest.raises(_abi.GnfError):
        binary_loss(emb, true.to("cpu"))
    with pytest.raises(ValueError):
        binary_loss(emb, true, max_nodes_per_graph=64, n_node_host=R.SIZES)   # the largest graph has 65 nodes
    with pytest.raises(ValueError):
        binary_loss(emb, true, max_nodes_per_graph=65537)
    with pytest.raises(NotImplementedError):
        binary_loss(emb, true, distance_fn=torch.sigmoid)


def test_an_empty_batch_gives_zeros():
    """n_nodes == 0 with two graphs, at the entry point itself: every output is zeroed, GNF_OK"""
    import ctypes as C
    from gnf_amd import _abi
    lib = _abi.lib()
    off = torch.zeros(3, dtype=torch.int32, device=DEV)
    loss = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    fp, fn = torch.full((2,), 7, dtype=torch.int64, device=DEV), torch.full((2,), 7, dtype=torch.int64, device=DEV)
    csr = _abi.GnfCsr(0, 0, 0, 0, off.data_ptr(), 2)
    spec = _abi.GnfAdjLossSpec(10.0, 1.0, 1, 0, 0.1, 0.5)
    with torch.cuda.device(DEV):
        _abi.check(lib.gnf_adj_loss_f32(C.byref(csr), None, 4, 4, 0, C.byref(spec), _abi.ptr(loss), _abi.ptr(sums), _abi.ptr(fp),
                                        _abi.ptr(fn), None, 4, 1.0, None, 0, _abi.stream_ptr(torch.device(DEV))),
                   "gnf_adj_loss_f32")
    torch.cuda.synchronize()
    assert loss.tolist() == [0.0, 0.0] == sums.tolist() and fp.tolist() == [0, 0] == fn.tolist()
