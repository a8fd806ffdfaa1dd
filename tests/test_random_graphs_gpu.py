"""The random graph models on the MI355X (include/gnf_random_graphs.h): every array of the raw entry points, written into
guard-banded buffers, integer for integer against the numpy twin AND the pure-Python restatement, and (rowptr, senders) against
gnf_build_csr of the edge list in both orientations; determinism and seeds; edge_capacity; the call replayed from a hipGraph with
the device seed word; then the consumers - the flow and the graph scores without a CSR build, connected components of
Barabasi-Albert graphs, the baselines of a data set and the example driver with --report_baselines."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

import random_graphs_ref as RR
from gnf_amd import _abi, gnn, random_graphs as G
from gnf_amd.graphs import build_csr_device, csr_of
from helpers import graph_from_arrays
from test_batches_gpu import Guarded, SENTINEL, _leave_the_process_wide_generators_as_found, _no_build   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 64, 65, 0, 129]          # both sides of a bitmap word's edge, the empty graph mid-batch, three words
MIXED = [64, 3, 65, 41, 128, 40, 130]       # both word-edge sizes beside graphs at, below and above m = 40
NEXT_TO_ZERO = 2.0 ** -32
KEYS = ("senders", "receivers", "rowptr", "n_edge")
MMD_ATOL = 1e-10   # the project's bound for a set against itself (tests/test_graph_stats_gpu.py)


def _t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _raw(model, sizes, par, par_out=None, n_blocks=1, blocks=None, max_m=64, seed=0, first_graph=0, self_loops=False, seed_dev=None,
         edges=None, cap=None):
    """gnf_random_graph_edges_count + gnf_adj_edges_fill into guard-banded outputs and a guard-banded workspace; `edges` entries
    for senders / receivers (default: the twin's total); returns the arrays and the twin's dict"""
    ba = model == "barabasi_albert"
    b, n = len(sizes), int(sum(sizes))
    used = seed if seed_dev is None else int(seed_dev[0])          # the twin draws with the seed the kernels will read
    want = G.random_graphs_host(model, sizes, par, par_out, n_blocks, blocks, used, first_graph, self_loops, max_m)
    e = want["total"] if edges is None else edges
    cap = max(max(sizes), 1) if cap is None else cap
    lib = _abi.lib()
    keep = [_t(np.asarray(sizes, np.int32))]
    spec = _abi.GnfRandomGraphSpec()
    spec.seed, spec.first_graph, spec.self_loops = int(seed) & (2 ** 64 - 1), first_graph, int(self_loops)
    spec.seed_dev = None if seed_dev is None else seed_dev.data_ptr()
    spec.model = _abi.GNF_RG_BARABASI_ALBERT if ba else _abi.GNF_RG_PLANTED
    if ba:
        keep.append(_t(np.broadcast_to(np.asarray(par, np.int32), (b,)).copy()))
        spec.m_dev, spec.max_m = keep[-1].data_ptr(), max_m
    else:
        keep.append(_t(np.asarray(par, np.uint64).view(np.int64)))
        spec.thr_in, spec.n_blocks = keep[-1].data_ptr(), n_blocks
        if par_out is not None:
            keep.append(_t(np.asarray(par_out, np.uint64).view(np.int64)))
            spec.thr_out = keep[-1].data_ptr()
        if blocks is not None:
            keep.append(_t(np.asarray(blocks, np.int32)))
            spec.block = keep[-1].data_ptr()
    ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, cap)
    out = Guarded([n + 1, b, 2, e, e], [17, 18, 16, 19, 21])        # (total: an int64 at an 8-byte aligned lead)
    ws = Guarded([(ws_bytes + 3) // 4], [64])
    rowptr, n_edge, total, snd, rcv = out.ptrs()
    st = _abi.stream_ptr(torch.device(DEV))
    _abi.check(lib.gnf_random_graph_edges_count(C.byref(spec), _abi.ptr(keep[0]), b, n, cap, rowptr, n_edge, total, ws.ptrs()[0],
                                                ws_bytes, st), "gnf_random_graph_edges_count")
    _abi.check(lib.gnf_adj_edges_fill(b, n, cap, rowptr, e, snd, rcv, ws.ptrs()[0], ws_bytes, st), "gnf_adj_edges_fill")
    torch.cuda.synchronize()
    out.check()
    ws.check()
    got = dict(zip(("rowptr", "n_edge", "total", "senders", "receivers"), out.views))
    got["total"] = int(got["total"].view(torch.int64)[0])
    return got, want


def _check(got, want, ref, sizes):
    for k in KEYS:
        assert got[k].dtype == torch.int32 and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
        assert want[k].tolist() == ref[k], k
    assert got["total"] == want["total"] == ref["total"]
    # (rowptr, senders) is gnf_build_csr of the edge list by receiver, and by sender as well
    n, e = int(sum(sizes)), want["total"]
    graph = graph_from_arrays(np.asarray(sizes, np.int32), want["n_edge"], got["senders"].cpu().numpy(),
                              got["receivers"].cpu().numpy(), np.zeros((n, 1), np.float32), DEV)
    by_r, by_s = build_csr_device(graph), build_csr_device(graph, by_sender=True)
    torch.cuda.synchronize()
    for csr in (by_r, by_s):
        assert torch.equal(csr.rowptr, got["rowptr"]) and torch.equal(csr.col[:e], got["senders"])


# ---- the arrays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("p", [0.0, NEXT_TO_ZERO, 0.3, 1.0])
def test_erdos_renyi_equals_twin_and_restatement(p, self_loops):
    b = len(SIZES)
    got, want = _raw("erdos_renyi", SIZES, G.thresholds(p, b), seed=12345, self_loops=self_loops)
    ref = RR.batch("planted", SIZES, [RR.threshold(p)] * b, seed=12345, self_loops=self_loops)
    _check(got, want, ref, SIZES)
    if p == 1.0:
        assert got["total"] == sum(n * n if self_loops else n * (n - 1) for n in SIZES)


@pytest.mark.parametrize("n_blocks", [1, 2, 3, "labels"])
def test_planted_partition_equals_twin_and_restatement(n_blocks):
    b, n = len(SIZES), sum(SIZES)
    blocks = (np.arange(n) * 7 % 5).astype(np.int32) if n_blocks == "labels" else None
    nb = 1 if blocks is not None else n_blocks
    p_in, p_out = np.linspace(0.2, 0.8, b), np.linspace(0.3, 0.0, b)
    kw = dict(n_blocks=nb, seed=2 ** 63 + 5, first_graph=9, self_loops=True)
    got, want = _raw("planted_partition", SIZES, G.thresholds(p_in, b), G.thresholds(p_out, b), blocks=blocks, **kw)
    ref = RR.batch("planted", SIZES, [RR.threshold(p) for p in p_in], [RR.threshold(p) for p in p_out],
                   blocks=None if blocks is None else blocks.tolist(), **kw)
    _check(got, want, ref, SIZES)


@pytest.mark.parametrize("m", [1, 2, 40, 64])
def test_barabasi_albert_equals_twin_and_restatement(m):
    b = len(SIZES)
    got, want = _raw("barabasi_albert", SIZES, [m] * b, seed=12345, self_loops=(m == 2))
    ref = RR.batch("ba", SIZES, [m] * b, seed=12345, self_loops=(m == 2))
    _check(got, want, ref, SIZES)
    assert want["n_edge"].tolist() == [(2 * m * (n - m) if n > m else 0) + (n if m == 2 else 0) for n in SIZES]


@pytest.mark.parametrize("n,m", [(44, 40), (70, 64)])
def test_barabasi_albert_fallback_on_the_device(n, m):
    got, want = _raw("barabasi_albert", [n] * 4, [m] * 4, seed=12345)
    ref = RR.batch("ba", [n] * 4, [m] * 4, seed=12345)
    assert all(f > 0 for f in ref["fallbacks"]), ref["fallbacks"]
    _check(got, want, ref, [n] * 4)


def test_a_mixed_batch_equals_twin_and_restatement():
    ms = [1, 40, 40, 40, 1, 40, 40]
    got, want = _raw("barabasi_albert", MIXED, ms, seed=99, first_graph=3, self_loops=True, max_m=40)
    _check(got, want, RR.batch("ba", MIXED, ms, seed=99, first_graph=3, self_loops=True), MIXED)
    # m above the host bound is clamped to it; a bound on the graph size larger than any graph changes nothing
    clamped, want5 = _raw("barabasi_albert", MIXED, [99] * 7, seed=99, max_m=5, cap=200)
    assert all(torch.equal(clamped[k].cpu(), torch.from_numpy(want5[k])) for k in KEYS)
    assert all(np.array_equal(want5[k], G.random_graphs_host("barabasi_albert", MIXED, [5] * 7, seed=99)[k]) for k in KEYS)
    b = len(MIXED)
    p_in, p_out = np.linspace(1.0, 0.1, b), np.linspace(0.0, 0.4, b)
    got, want = _raw("planted_partition", MIXED, G.thresholds(p_in, b), G.thresholds(p_out, b), n_blocks=2, seed=99, cap=200)
    ref = RR.batch("planted", MIXED, [RR.threshold(p) for p in p_in], [RR.threshold(p) for p in p_out], n_blocks=2, seed=99)
    _check(got, want, ref, MIXED)


def test_two_calls_give_the_same_bits_and_seeds_differ():
    b = len(MIXED)
    for model, par in (("erdos_renyi", G.thresholds(0.3, b)), ("barabasi_albert", [3] * b)):
        a, _ = _raw(model, MIXED, par, seed=424242)
        again, _ = _raw(model, MIXED, par, seed=424242)
        word = torch.tensor([424242], dtype=torch.int64, device=DEV)
        by_word, _ = _raw(model, MIXED, par, seed=0, seed_dev=word)               # the word wins over the value
        other, _ = _raw(model, MIXED, par, seed=424243)
        for k in KEYS:
            assert torch.equal(a[k], again[k]) and torch.equal(a[k], by_word[k]), (model, k)
        assert int(word[0]) == 424242                                              # the kernels never write the seed word
        assert not torch.equal(a["senders"], other["senders"]) and not torch.equal(a["rowptr"], other["rowptr"])   # other edges
        for lo, hi in ((0, 64), (67, 132), (341, 471)):                            # ... in every graph large enough to tell
            assert not torch.equal(a["rowptr"][lo + 1:hi + 1] - a["rowptr"][lo], other["rowptr"][lo + 1:hi + 1] - other["rowptr"][lo])
        # two calls of half a batch with first_graph
        lo, _ = _raw(model, MIXED[:3], par[:3], seed=424242)
        hi, _ = _raw(model, MIXED[3:], par[3:], seed=424242, first_graph=3)
        assert a["n_edge"].tolist() == lo["n_edge"].tolist() + hi["n_edge"].tolist()
        assert torch.equal(a["senders"], torch.cat([lo["senders"], hi["senders"] + sum(MIXED[:3])]))


def test_edge_capacity_below_the_total_keeps_the_first_edges():
    b = len(MIXED)
    for model, par in (("erdos_renyi", G.thresholds(0.3, b)), ("barabasi_albert", [3] * b)):
        full, want = _raw(model, MIXED, par, seed=7)
        k = want["total"] // 2 + 1
        cut, _ = _raw(model, MIXED, par, seed=7, edges=k)                         # the guards behind entry k are checked inside
        assert cut["total"] == want["total"] and torch.equal(cut["rowptr"], full["rowptr"])
        assert torch.equal(cut["senders"], full["senders"][:k]) and torch.equal(cut["receivers"], full["receivers"][:k])
        over, _ = _raw(model, MIXED, par, seed=7, edges=want["total"] + 11)       # more room than edges: the rest is not touched
        assert torch.equal(over["senders"][:want["total"]], full["senders"])
        assert bool((over["senders"][want["total"]:] == SENTINEL).all())


def test_a_captured_call_replays_with_the_seed_of_the_moment():
    sizes, s0 = [30, 65, 64, 7], 9000
    n = sum(sizes)
    nn = _t(np.asarray(sizes, np.int32))
    word = torch.tensor([s0], dtype=torch.int64, device=DEV)
    nodes = torch.zeros(n, 1, device=DEV)
    for make, par in ((G.erdos_renyi, _t(np.asarray([0.2, 0.5, 0.1, 0.9]))), (G.barabasi_albert, _t(np.asarray([2, 5, 1, 3], np.int32)))):
        eager = [make(sizes, par.cpu().numpy(), seed=s0 + k, device=DEV) for k in range(3)]
        room = max(int(r["total_edges"]) for r in eager) + 5
        word.fill_(s0)

        def launch():
            out = make(nn, par, seed_dev=word, nodes=nodes, max_nodes_per_graph=65, edge_capacity=room)
            word.add_(1)
            return out
        launch()                                                    # once eagerly (this consumes seed s0 - put it back)
        word.fill_(s0)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            out = launch()
        for k in range(3):
            cg.replay()
            torch.cuda.synchronize()
            e = int(eager[k]["total_edges"])
            assert int(out["total_edges"]) == e, k
            assert torch.equal(out["graph"].senders[:e], eager[k]["graph"].senders), k
            assert torch.equal(out["graph"].receivers[:e], eager[k]["graph"].receivers), k
            assert torch.equal(out["csr"].rowptr, eager[k]["csr"].rowptr) and torch.equal(out["graph"].n_edge, eager[k]["graph"].n_edge)
        assert int(word[0]) == s0 + 3


# ---- consumers ---------------------------------------------------------------------------------------------------------------------
def test_the_flow_and_the_scores_launch_no_csr_build(monkeypatch):
    from gnf_amd.graph_stats import graph_stats
    x = torch.randn(sum(MIXED), 2, device=DEV)
    made = [G.erdos_renyi(MIXED, 0.2, seed=3, self_loops=True, nodes=x), G.barabasi_albert(MIXED, 3, seed=3, self_loops=True, nodes=x),
            G.planted_partition(MIXED, 0.6, 0.05, n_blocks=3, seed=3, self_loops=True, nodes=x)]
    gnn.set_random_seed(5)
    mlp = partial(gnn.make_mlp_model, 16, 1, 2, gnn.leaky_relu, 0.1, 0.1)
    net = gnn.GRevNet(partial(gnn.avg_then_mlp_gnn, mlp, 1.0), 2, 2)
    _no_build(monkeypatch)
    for out in made:
        g = out["graph"]
        assert csr_of(g) is out["csr"] and csr_of(g, by_sender=True) is out["csr"]
        z_graph, logdet = net.f(g)
        stats = graph_stats(g)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(z_graph.nodes).all()) and bool(torch.isfinite(logdet).all())
        e = int(out["total_edges"])
        assert int(stats["n_edges"].sum()) == (e - sum(MIXED)) // 2 and g.senders.shape == (e,)
        # the same forward on a host-built copy of the edge list (its CSR from gnf_build_csr) gives the same bits
    monkeypatch.undo()
    g = made[0]["graph"]
    copy = graph_from_arrays(np.asarray(MIXED, np.int32), g.n_edge.cpu().numpy(), g.senders.cpu().numpy(), g.receivers.cpu().numpy(),
                             x.cpu().numpy(), DEV)
    assert torch.equal(net.f(copy)[0].nodes, net.f(g)[0].nodes)


def test_barabasi_albert_graphs_are_connected():
    from gnf_amd.graph_stats import graph_components
    sizes, ms = [41, 64, 2, 130, 65, 5, 200], [40, 1, 1, 64, 7, 4, 16]                # every graph has n > m
    out = G.barabasi_albert(sizes, ms, seed=12345)
    parts = graph_components(out["graph"])
    assert parts["n_components"].tolist() == [1] * len(sizes)
    assert parts["largest_component_size"].tolist() == sizes
    assert out["graph"].n_edge.tolist() == [2 * m * (n - m) for n, m in zip(sizes, ms)]
    # n <= m: every node is its own component
    lone = graph_components(G.barabasi_albert([5, 3], [5, 9], seed=1)["graph"])
    assert lone["n_components"].tolist() == [5, 3]


@pytest.fixture(scope="module")
def caveman():
    from gnf_amd import datasets as D
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    ds = D.GraphDataset("graph_rnn_community_small", 1)
    return tuple(data_dicts_to_graphs_tuple(ds.all.data_dicts(ids, ds._features), DEV) for ids in (ds.train_ids, ds.test_ids))


def test_baselines_of_a_data_set(caveman):
    from gnf_amd.graph_stats import graph_stats
    train, test = caveman
    rows = G.evaluate_baselines(train, test, seed=1)
    assert list(rows) == ["erdos_renyi", "barabasi_albert"]
    for model, row in rows.items():
        for k in ("degree_mmd", "clustering_mmd"):
            print(f"{model} {k}: {float(row[k]):.6f}")
            assert row[k].dtype == torch.float64 and np.isfinite(float(row[k])) and float(row[k]) >= -MMD_ATOL, (model, k)
    # one baseline graph per training graph, of its size, with the fitted parameter
    made = G.baselines(train, seed=1)
    stats = graph_stats(train)
    for model in ("erdos_renyi", "barabasi_albert"):
        assert torch.equal(made[model]["graph"].n_node.cpu(), train.n_node.cpu().to(torch.int32))
    m = G.fit_baseline(train, "barabasi_albert").to(torch.int64)
    n = train.n_node.to(DEV, torch.int64)
    assert torch.equal(graph_stats(made["barabasi_albert"]["graph"])["n_edges"], m * (n - m))
    p = G.fit_baseline((stats, train.n_node), "erdos_renyi")
    assert torch.equal(p, stats["n_edges"].double() / (n * (n - 1) // 2).double())
    # the fitted G(n, p) has the training set's edge count within 5 sigma of Binomial(pairs_b, p_b) summed over the graphs
    sigma = float((p * (1.0 - p) * (n * (n - 1) // 2).double()).sum().sqrt())
    got, want = int(graph_stats(made["erdos_renyi"]["graph"])["n_edges"].sum()), int(stats["n_edges"].sum())
    assert abs(got - want) <= 5 * sigma, (got, want, sigma)


def test_a_baseline_against_itself_scores_zero():
    from gnf_amd.graph_stats import evaluate_generated
    for out in (G.erdos_renyi([20, 33, 9, 64], 0.2, seed=2), G.barabasi_albert([20, 33, 9, 64], [2, 3, 1, 4], seed=2)):
        g = out["graph"]
        same = evaluate_generated(g, g, orbits=True, spectral=True)
        assert float(same["orbit_mmd"]) == 0.0 and float(same["spectral_mmd"]) == 0.0
        assert abs(float(same["degree_mmd"])) <= MMD_ATOL and abs(float(same["clustering_mmd"])) <= MMD_ATOL


def test_the_data_example_reports_baselines():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_grevnet_with_data.py"), "--make_chunks",
                          "--dataset", "graph_rnn_community_small", "--attn_type", "avg_then_mlp", "--node_embedding_dim", "8",
                          "--latent_dim", "16", "--num_layers", "2", "--num_coupling_layers", "2", "--train_batch_size", "4",
                          "--num_train_iters", "2", "--log_every_n_steps", "1", "--sample_size", "4", "--report_baselines"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows = dict(re.findall(r"^  (\S+)\s+degree_mmd (\S+) clustering_mmd \S+$", run.stdout, flags=re.M))
    assert list(rows) == ["model", "erdos_renyi", "barabasi_albert"], run.stdout[-1500:]
    assert all(np.isfinite(float(v)) for v in rows.values())
