"""gnf_amd.graph_stats.graph_components / keep_subgraphs (gnf_graph_components, gnf_graph_subgraph_count / _fill) on the MI355X
against the union-find reference of tests/graph_components_ref.py (itself checked against a second construction in
tests/test_graph_components_cpu.py).

Every output is an integer with a canonical definition (a component's label is its smallest node, edges come in one order), so
every comparison is for EQUALITY; there is no tolerance anywhere in this file.  The cases are the smallest that reach each
hazard: graph sizes on both sides of the 64-column word (63, 64, 65, 128, 129) with empty graphs between and behind them,
searches of 65 to 130 levels across two word edges, a hub in the last column, a single edge that spans a word edge, the tie
rule, no edges at all and every edge - each in the three spellings of an edge list the graph model merges - and two graphs
past the sizes at which the kernels' loops take a second turn (more than 64 and more than 256 words per row)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_graphs_ref as DR
import graph_components_ref as R
from helpers import graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPELLINGS = ["symmetric", "one_direction", "duplicates_and_loops"]
BATCHES = {"word_edges": R.word_edge_cases, "hazards": R.hazard_cases}
SUB_KEYS = ("new_id", "node_index", "new_n_node", "n_edge", "rowptr", "senders", "receivers")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _spell(cases, how, rng=None, d=1):
    """One GraphsTuple spelling of [(name, n, (s, r) local, one direction)]: edges stay grouped by graph."""
    n_node, n_edge, ss, rr, off = [], [], [], [], 0
    for _, n, (s, r) in cases:
        s, r = np.asarray(s, np.int64), np.asarray(r, np.int64)
        if how == "symmetric":
            s, r = np.concatenate([s, r]), np.concatenate([r, s])
        elif how == "duplicates_and_loops":
            loops = np.arange(n)
            s, r = np.concatenate([s, r, s, loops, loops]), np.concatenate([r, s, r, loops, loops])
            p = rng.permutation(len(s))
            s, r = s[p], r[p]
        else:
            assert how == "one_direction"
        n_node.append(n), n_edge.append(len(s)), ss.append(s + off), rr.append(r + off)
        off += n
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    x = np.arange(off * d, dtype=np.float32).reshape(off, d)        # row i holds i d ..: index_select is visible in the nodes
    return graph_from_arrays(n_node, n_edge, cat(ss), cat(rr), x, DEV)


@pytest.fixture(scope="module")
def ref():
    """per batch: the cases, their reference batch (n_node, s, r) and the reference components - computed once, never edited"""
    out = {}
    for name, make in list(BATCHES.items()) + [("all", R.all_cases)]:
        cases = make()
        flat = R.batch(cases)
        out[name] = {"cases": cases, "flat": flat, "want": R.components(*flat)}
    return out


def _assert_components(out, want, what=""):
    from gnf_amd.graph_stats import COMPONENT_KEYS
    assert tuple(out) == COMPONENT_KEYS == R.KEYS
    for k in R.KEYS:
        assert out[k].dtype == torch.int32 and out[k].device.type == "cuda", k
        np.testing.assert_array_equal(out[k].cpu().numpy(), want[k], err_msg=f"{what} {k}")


def _sub_arrays(res):
    g = res["graph"]
    got = {"new_id": res["new_id"], "node_index": res["node_index"], "new_n_node": g.n_node, "n_edge": g.n_edge,
           "rowptr": res["csr"].rowptr, "senders": g.senders, "receivers": g.receivers}
    assert all(v.dtype == torch.int32 and v.device.type == "cuda" for v in got.values())
    assert res["total_nodes"].dtype == res["total_edges"].dtype == torch.int64 and res["total_nodes"].dim() == 0
    return {k: v.cpu().numpy() for k, v in got.items()}


def _assert_subgraph(res, want, what=""):
    got = _sub_arrays(res)
    for k in SUB_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    assert int(res["total_nodes"]) == len(want["node_index"]) and int(res["total_edges"]) == len(want["senders"]), what


# ---- 1. components: every case in every spelling ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", SPELLINGS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_components_equal_the_reference(ref, batch, how):
    from gnf_amd.graph_stats import graph_components
    r = ref[batch]
    g = _spell(r["cases"], how, np.random.default_rng(7))
    out = graph_components(g)
    for k in R.KEYS[2:]:
        print(batch, how, k, out[k].cpu().tolist())
    _assert_components(out, r["want"], f"{batch} {how}")
    again = graph_components(g)                                   # two calls give the same bits
    assert all(torch.equal(again[k], out[k]) for k in R.KEYS)


def test_hazard_cases_are_what_they_claim(ref):
    w, names = ref["hazards"]["want"], [c[0] for c in ref["hazards"]["cases"]]
    at = {n: k for k, n in enumerate(names)}
    for p in ("path130", "path130_reversed", "path130_folded"):
        assert w["n_components"][at[p]] == 1 and w["largest_component_size"][at[p]] == 130
    assert w["n_components"][at["tie"]] == 4 and w["n_isolated"][at["isolated70"]] == 70 and w["n_components"][at["empty"]] == 0
    assert w["largest_component_root"][at["empty"]] == -1 and w["n_isolated"][at["edge_63_64"]] == 63
    ww = ref["word_edges"]["want"]
    assert [n for _, n, _ in ref["word_edges"]["cases"]] == [1, 2, 63, 64, 0, 65, 128, 129, 0]
    assert (ww["n_components"][[2, 3, 5, 6, 7]] > 5).all() and (ww["largest_component_size"][[2, 3, 5, 6, 7]] > 2).all()


def test_bounds_above_the_largest_graph_and_sizes_on_the_host(ref):
    from gnf_amd.graph_stats import graph_components
    r = ref["all"]
    g = _spell(r["cases"], "one_direction")
    for kw in ({"max_nodes_per_graph": 200}, {"max_nodes_per_graph": 130}, {"n_node_host": [n for _, n, _ in r["cases"]]},
               {"max_nodes_per_graph": 65536}):
        _assert_components(graph_components(g, **kw), r["want"], str(kw))


def test_graphs_without_nodes_and_an_empty_batch():
    from gnf_amd.graph_stats import graph_components, keep_subgraphs
    for sizes in ([0, 0, 0], []):
        g = graph_from_arrays(sizes, [0] * len(sizes), [], [], np.zeros((0, 2), np.float32), DEV)
        out = graph_components(g)
        _assert_components(out, R.components(sizes, [], []), str(sizes))
        assert out["largest_component_root"].tolist() == [-1] * len(sizes)
        for keep in R.RULES:
            res = keep_subgraphs(g, keep, self_loops=True)
            _assert_subgraph(res, R.subgraph(sizes, [], [], np.zeros(0, bool), True), f"{sizes} {keep}")
            assert res["graph"].nodes.shape == (0, 2)


# ---- 2. extraction ---------------------------------------------------------------------------------------------------------
def _keep_argument(rule, n, dtype=torch.bool):
    """(keep_subgraphs' argument, the reference's rule and mask): the mask is seeded, about two nodes in three"""
    if rule != "mask":
        return rule, rule, None
    m = np.random.default_rng(2026).random(n) < 0.66
    return torch.as_tensor(m).to(DEV).to(dtype), "mask", m


@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("rule", ["largest_component", "non_isolated", "mask"])
def test_subgraphs_equal_the_reference(ref, rule, self_loops):
    from gnf_amd.graphs import csr_of
    from gnf_amd.graph_stats import STATS_KEYS, graph_stats, keep_subgraphs
    r = ref["all"]
    n_node, s, t = r["flat"]
    n = sum(n_node)
    g = _spell(r["cases"], "duplicates_and_loops", np.random.default_rng(11), d=3)
    arg, ref_rule, mask = _keep_argument(rule, n, torch.uint8 if self_loops else torch.bool)
    keep = R.keep_mask(n_node, s, t, ref_rule, mask)
    want = R.subgraph(n_node, s, t, keep, self_loops)
    assert 0 < len(want["node_index"]) < n and len(want["senders"]) > 100        # something kept, something dropped
    res = keep_subgraphs(g, arg, self_loops=self_loops)
    _assert_subgraph(res, want, f"{rule} loops={self_loops}")
    again = _sub_arrays(keep_subgraphs(g, arg, self_loops=self_loops))             # two calls give the same bits
    assert all(np.array_equal(again[k], v) for k, v in _sub_arrays(res).items())
    kept = res["graph"]
    assert len(kept.n_node) == len(n_node) and kept.globals is g.globals and not kept.edges.any()
    assert kept.edges.shape == kept.senders.shape
    assert torch.equal(kept.nodes, g.nodes[torch.as_tensor(want["node_index"]).long().to(DEV)])
    for by_sender in (False, True):
        assert csr_of(kept, by_sender=by_sender) is res["csr"]
    # the scores accept the batch as it is, and see the reference's subgraph
    twin = graph_from_arrays(want["new_n_node"], want["n_edge"], want["senders"], want["receivers"],
                             np.zeros((len(want["node_index"]), 1), np.float32), DEV)
    a, b = graph_stats(kept, max_nodes_per_graph=130), graph_stats(twin, max_nodes_per_graph=130)
    for k in STATS_KEYS:
        assert torch.equal(a[k], b[k]), k
    if rule == "largest_component" and not self_loops:                         # the other spellings and a bound: the same bits
        for how in SPELLINGS[:2]:
            other = keep_subgraphs(_spell(r["cases"], how, d=3), rule, max_nodes_per_graph=200)
            _assert_subgraph(other, want, how)


def test_graphs_of_more_than_64_and_more_than_256_words():
    """4 200 nodes: the frontier's words no longer fit one 64-lane read; 16 500 nodes: a thread owns more than one word of the
    bitsets and the rank scan more than one word per thread.  Hundreds of searches per graph, edges that join neighbouring
    words, roots past the first word."""
    from gnf_amd.graph_stats import graph_components, keep_subgraphs
    cases = R.large_cases()
    n_node, s, t = R.batch(cases)
    want = R.components(n_node, s, t)
    g = _spell(cases, "one_direction")
    _assert_components(graph_components(g), want, "large")
    _assert_components(graph_components(_spell(cases, "symmetric"), max_nodes_per_graph=65536), want, "large, bound 65536")
    for rule, loops in (("largest_component", False), ("non_isolated", True)):
        sub = R.subgraph(n_node, s, t, R.keep_mask(n_node, s, t, rule), loops)
        _assert_subgraph(keep_subgraphs(g, rule, self_loops=loops), sub, f"large {rule}")


def test_a_connected_batch_comes_back_whole(community_medium):
    from gnf_amd.graph_stats import graph_components, keep_subgraphs
    nn, ne, s, r = O.batch_graphs(*community_medium, list(range(8)))
    n = int(np.sum(nn))
    g = graph_from_arrays(nn, ne, s, r, np.zeros((n, 1), np.float32), DEV)
    c = graph_components(g)
    assert c["n_components"].tolist() == [1] * 8 and not c["n_isolated"].any()
    assert torch.equal(c["largest_component_size"], g.n_node)
    want = R.subgraph(nn, s, r, np.ones(n, bool))
    for keep in R.RULES:
        res = keep_subgraphs(g, keep)
        _assert_subgraph(res, want, keep)
        assert torch.equal(res["node_index"], torch.arange(n, dtype=torch.int32, device=DEV))
        assert torch.equal(res["graph"].n_node, g.n_node)


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
def test_decode_then_components_then_keep_then_flow(monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs, log_prob_terms
    from gnf_amd.graph_stats import evaluate_generated, graph_components, graph_stats, hist_mmd, keep_subgraphs
    n_node = [1, 12, 0, 33, 70]
    z, labels = DR.clustered_embeddings(np.random.default_rng(3), n_node, 8)
    closed = DR.edges_from_blocks(DR.clique_blocks(n_node, labels), 0.5, False)      # what the decoder must produce
    want = R.components(n_node, closed["senders"], closed["receivers"])
    assert want["n_components"].tolist()[0] == 1 and want["n_components"][2] == 0 and (want["n_components"][[1, 3, 4]] >= 2).all()
    shell = graph_from_arrays(n_node, np.zeros(len(n_node), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)
    graph = decode_graphs(shell)["graph"]
    np.testing.assert_array_equal(graph.senders.cpu().numpy(), closed["senders"])

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR was seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    _assert_components(graph_components(graph), want, "decoded")
    keep = R.keep_mask(n_node, closed["senders"], closed["receivers"], "largest_component")
    sub = R.subgraph(n_node, closed["senders"], closed["receivers"], keep, True)
    res = keep_subgraphs(graph, "largest_component", self_loops=True)
    _assert_subgraph(res, sub, "decoded")
    kept = res["graph"]
    again = graph_components(kept)                                                    # one component per graph is left
    assert again["n_components"].tolist() == [1, 1, 0, 1, 1] and torch.equal(again["largest_component_size"], kept.n_node)
    hp = dict(D=8, latent=16, K=2, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
    p = O.make_grevnet_params(3, 4, 16, 2, 2, final_scale=0.5)
    out = log_prob_terms(make_product_grevnet(hp, p), kept)
    torch.cuda.synchronize()
    n = len(sub["node_index"])
    ref = O.Fp64Dense(sub["senders"], sub["receivers"], n, agg="mean", combine="agg", epsilon=1.0,
                      activation="leaky_relu").log_prob(z[sub["node_index"]], p, 2)
    np.testing.assert_allclose(out["z_graph"].nodes.cpu().numpy(), ref["z"], atol=1e-4, rtol=1e-4)     # the project's bound
    assert abs(float(out["log_prob_xs_per_node"]) - ref["log_prob_xs_per_node"]) <= 1e-4
    # evaluate_generated(keep=...) scores the reduced batch, the reference batch as given
    plain = evaluate_generated(graph, graph)
    cut = evaluate_generated(graph, graph, keep="largest_component")
    # (the float64 reference gives 0 and 0.276 here; a set against itself is 0 up to the rounding of three block sums)
    assert abs(float(plain["degree_mmd"])) <= 1e-12 and float(cut["degree_mmd"]) > 0.1
    a, b = graph_stats(keep_subgraphs(graph, "largest_component")["graph"], clustering_bins=100), graph_stats(graph, clustering_bins=100)
    assert torch.equal(cut["degree_mmd"], hist_mmd(a["degree_hist"], b["degree_hist"], "gaussian_emd", 1.0, 1.0))
    with pytest.raises(ValueError):
        evaluate_generated(b, graph, keep="largest_component")


def test_generate_graphs_with_keep_changes_nothing_else(grid_small):
    from gnf_amd.flow import generate_graphs
    from gnf_amd.graphs import csr_of
    nn, ne, s, r = O.batch_graphs(*grid_small, [6, 7])
    nn3, ne3 = np.array([nn[0], 0, nn[1]]), np.array([ne[0], 0, ne[1]])      # an empty graph in the middle
    n = int(nn3.sum())
    hp = dict(D=8, latent=16, K=3, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
    net = make_product_grevnet(hp, O.make_grevnet_params(2, 4, 16, 3, 2, final_scale=0.5))
    shell = graph_from_arrays(nn3, ne3, s, r, np.zeros((n, 8), np.float32), DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(1)
    for loops in (False, True):
        base = generate_graphs(net, shell, generator=gen(), self_loops=loops)
        assert "kept" not in base
        for keep in R.RULES:
            out = generate_graphs(net, shell, generator=gen(), self_loops=loops, keep=keep)
            assert set(out) == set(base) | {"kept"}
            for k, v in base.items():
                if isinstance(v, torch.Tensor):
                    assert torch.equal(out[k], v), k
            for f in ("nodes", "senders", "receivers", "n_node", "n_edge"):
                assert torch.equal(getattr(out["graph"], f), getattr(base["graph"], f)), f
            assert torch.equal(out["csr"].rowptr, base["csr"].rowptr)
            dec = out["graph"]
            ss, rr = dec.senders.cpu().numpy(), dec.receivers.cpu().numpy()
            want = R.subgraph(nn3, ss, rr, R.keep_mask(nn3, ss, rr, keep), loops)
            _assert_subgraph(out["kept"], want, f"{keep} loops={loops}")
            assert csr_of(out["kept"]["graph"]) is out["kept"]["csr"]


# ---- 4. reproducibility and capture ----------------------------------------------------------------------------------------
def _mirrored(cases):
    """every graph renumbered back to front (i -> n - 1 - i): the same sizes and edge counts, other rows, other labels"""
    return [(name, n, (n - 1 - np.asarray(s, np.int64), n - 1 - np.asarray(r, np.int64))) for name, n, (s, r) in cases]


def test_graph_components_replays_on_a_second_batch_in_the_same_buffers(ref):
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured with
    torch.cuda.graph (one stream, no branches) on CSR buffers that hold the first batch, the second batch (same sizes, every
    graph mirrored) is copied into those buffers, and the replay equals the eager call on the second batch."""
    from gnf_amd.graphs import Csr, csr_of, seed_csr_cache
    from gnf_amd.graph_stats import graph_components
    cases = ref["hazards"]["cases"]
    first, second = _spell(cases, "symmetric"), _spell(_mirrored(cases), "symmetric")
    want_second = R.components(*R.batch(_mirrored(cases)))
    assert not np.array_equal(want_second["component"], ref["hazards"]["want"]["component"])
    eager = [graph_components(g, max_nodes_per_graph=200) for g in (first, second)]
    _assert_components(eager[0], ref["hazards"]["want"], "first")
    _assert_components(eager[1], want_second, "second")
    ca, cb = csr_of(first), csr_of(second)
    assert ca.n_edges == cb.n_edges and torch.equal(first.n_node, second.n_node)
    rowptr, col = ca.rowptr.clone(), ca.col.clone()
    held = first.replace(senders=first.senders.clone(), receivers=first.receivers.clone())     # a key of its own in the cache
    seed_csr_cache(held, Csr(rowptr, col, ca.n_nodes, ca.n_edges))
    warm = graph_components(held, max_nodes_per_graph=200)          # (also the offsets cache of this n_node tensor)
    assert all(torch.equal(warm[k], eager[0][k]) for k in R.KEYS)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = graph_components(held, max_nodes_per_graph=200)
    for src, want in ((cb, eager[1]), (ca, eager[0]), (cb, eager[1])):
        rowptr.copy_(src.rowptr), col.copy_(src.col)
        for k in R.KEYS:
            captured[k].fill_(77)
        cg.replay()
        torch.cuda.synchronize()
        for k in R.KEYS:
            assert torch.equal(captured[k], want[k]), k


# ---- 5. raw entry points ---------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched_and_capacities_hold(ref):
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    r = ref["all"]
    n_node, s, t = r["flat"]
    g = _spell(r["cases"], "symmetric")
    n, b = int(g.nodes.shape[0]), int(g.n_node.shape[0])
    desc = csr_desc(g, csr_of(g), node_offsets=True)
    st = _abi.stream_ptr(torch.device(DEV))
    full = lambda k, dt=torch.int32: torch.full((k,), 77, dtype=dt, device=DEV)
    per_node, per_graph = [full(n), full(n)], [full(b) for _ in range(4)]
    ws_bytes = lib.gnf_graph_subgraph_workspace_bytes(b, n, 130)
    assert ws_bytes >= lib.gnf_graph_components_workspace_bytes(b, n, 130) > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    comp = lambda cap, bytes_: lib.gnf_graph_components(C.byref(desc), cap, *(_abi.ptr(x) for x in per_node + per_graph),
                                                        _abi.ptr(ws), bytes_, st)
    assert comp(-1, ws_bytes) == -2 and comp(65537, ws_bytes) == -2 and comp(130, 8) == -3
    new_id, new_n, rowptr, n_edge, totals = full(n), full(b), full(n + 1), full(b), full(2, torch.int64)
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    count = lambda cap, rule, m, loops, bytes_: lib.gnf_graph_subgraph_count(
        C.byref(desc), cap, rule, _abi.ptr(m), loops, _abi.ptr(new_id), _abi.ptr(new_n), _abi.ptr(rowptr), _abi.ptr(n_edge),
        _abi.ptr(totals), _abi.ptr(ws), bytes_, st)
    assert count(130, 2, None, 0, ws_bytes) == -1 and count(130, 3, mask, 0, ws_bytes) == -1 and count(130, 0, None, 2, ws_bytes) == -1
    assert count(-1, 0, None, 0, ws_bytes) == -2 and count(130, 0, None, 0, ws_bytes - 1) == -3
    torch.cuda.synchronize()
    for x in per_node + per_graph + [new_id, new_n, rowptr, n_edge, totals]:
        assert (x == 77).all()
    # a real count, then a fill with room for fewer rows and edges than there are: nothing is written past either capacity
    want = R.subgraph(n_node, s, t, R.keep_mask(n_node, s, t, "non_isolated"), True)
    assert count(130, 1, None, 1, ws_bytes) == 0
    n_new, e_new = totals.tolist()
    assert (n_new, e_new) == (len(want["node_index"]), len(want["senders"]))
    np.testing.assert_array_equal(rowptr[:n_new + 1].cpu().numpy(), want["rowptr"])
    assert (rowptr[n_new + 1:] == 77).all()
    ncap, ecap = n_new - 3, e_new - 5
    index, snd, rcv = full(n_new), full(e_new), full(e_new)
    fill = lambda nc, ec, bytes_: lib.gnf_graph_subgraph_fill(b, n, 130, _abi.ptr(rowptr), nc, ec, _abi.ptr(index), _abi.ptr(snd),
                                                              _abi.ptr(rcv), _abi.ptr(ws), bytes_, st)
    assert fill(-1, ecap, ws_bytes) == -2 and fill(ncap, ecap, ws_bytes - 1) == -3
    torch.cuda.synchronize()
    assert (index == 77).all() and (snd == 77).all() and (rcv == 77).all()
    assert fill(ncap, ecap, ws_bytes) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(index[:ncap].cpu().numpy(), want["node_index"][:ncap])
    np.testing.assert_array_equal(snd[:ecap].cpu().numpy(), want["senders"][:ecap])
    np.testing.assert_array_equal(rcv[:ecap].cpu().numpy(), want["receivers"][:ecap])
    assert (index[ncap:] == 77).all() and (snd[ecap:] == 77).all() and (rcv[ecap:] == 77).all()
