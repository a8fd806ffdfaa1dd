"""gnf_amd.graph_stats (gnf_graph_stats, gnf_hist_mmd_f64) on the MI355X against tests/graph_stats_ref.py.

Integer outputs (degree, triangles, both histograms, n_edges, n_triangles) are asserted EQUAL - nothing is excluded.
MMD^2 is held to an absolute error of 1e-10 against the float64 reference: each kernel value k in [0, 1] carries at most
about L 2^-53 relative error in W (prefix sums in another order), damped by u e^-u <= 1 / e, so <~ 5e-14 per k at L <= 512, and
MMD^2 is a +- combination of four means of such values, about 2e-13; 1e-10 leaves more than 100x headroom and is seven orders
below any MMD of interest.  The reduction is also bit-reproducible: two calls return identical bits."""
import math

import numpy as np
import pytest
import torch

import decode_graphs_ref as DR
import graph_stats_ref as R
from helpers import graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_KEYS = ("degree", "triangles", "degree_hist", "clustering_hist", "n_edges", "n_triangles")
DTYPES = {"degree": torch.int32, "triangles": torch.int32, "degree_hist": torch.int32, "clustering_hist": torch.int32,
          "n_edges": torch.int64, "n_triangles": torch.int64, "clustering": torch.float64}
MMD_ATOL = 1e-10
DECODE_N_NODE = [1, 63, 64, 65, 130, 0, 17]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _graph(n_node, n_edge, s, r):
    return graph_from_arrays(n_node, n_edge, s, r, np.zeros((int(np.sum(n_node)), 1), np.float32), DEV)


def _host(stats):
    for k, dt in DTYPES.items():
        assert stats[k].dtype == dt and stats[k].device.type == "cuda", k
    return {k: v.cpu().numpy() for k, v in stats.items()}


def _assert_stats(got, want, what=""):
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")
    np.testing.assert_allclose(got["clustering"], want["clustering"], rtol=1e-15, atol=0, err_msg=what)


def _spell(graphs, how, rng):
    """One GraphsTuple spelling of [(n, (s, r) local, one direction)]: edges stay grouped by graph (the block-diagonal layout)."""
    n_node, n_edge, ss, rr, off = [], [], [], [], 0
    for n, (s, r) in graphs:
        s, r = np.asarray(s, np.int64), np.asarray(r, np.int64)
        if how == "both_loops_shuffled":
            loops = np.arange(n)
            s, r = np.concatenate([s, r, loops]), np.concatenate([r, s, loops])
            p = rng.permutation(len(s))
            s, r = s[p], r[p]
        elif how == "duplicated":
            s, r = np.concatenate([s, s]), np.concatenate([r, r])
        else:
            assert how == "one_direction"
        n_node.append(n), n_edge.append(len(s)), ss.append(s + off), rr.append(r + off)
        off += n
    return _graph(n_node, n_edge, np.concatenate(ss), np.concatenate(rr))


@pytest.fixture(scope="module")
def mixed():
    """Sizes on the 64-column word boundaries, three words and an empty graph; K65, a star, a cycle, G(130, 0.3)."""
    rng = np.random.default_rng(20240)
    graphs = [(1, R.complete(1)), (2, R.complete(2)), (3, R.complete(3)), (63, R.cycle(63)), (64, R.star(64)),
              (65, R.complete(65)), (130, R.gnp(130, 0.3, rng)), (0, R.complete(0)), (17, R.gnp(17, 0.5, rng))]
    assert [n for n, _ in graphs] == [1, 2, 3, 63, 64, 65, 130, 0, 17]
    n_node, s, r = R.batch(graphs)
    want = R.graph_stats(n_node, s, r)
    assert want["triangles"][1 + 2 + 3 + 63 + 64] == math.comb(64, 2) and want["n_triangles"][6] > 1000
    return {"graphs": graphs, "n_node": n_node, "want": want}


@pytest.fixture(scope="module")
def decoded():
    """decode_graphs(...)["graph"] of clustered embeddings (as in test_decode_graphs_gpu.py) and the reference on its host copy"""
    from gnf_amd.flow import decode_graphs
    z, _ = DR.clustered_embeddings(np.random.default_rng(3), DECODE_N_NODE, 3)
    shell = graph_from_arrays(DECODE_N_NODE, np.zeros(len(DECODE_N_NODE), np.int32), np.zeros(0, np.int32),
                              np.zeros(0, np.int32), z, DEV)
    graph = decode_graphs(shell, self_loops=True)["graph"]
    s, r = graph.senders.cpu().numpy(), graph.receivers.cpu().numpy()
    assert len(s) > sum(DECODE_N_NODE)
    return {"graph": graph, "want": R.graph_stats(DECODE_N_NODE, s, r)}


# ---- 1. integer outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["both_loops_shuffled", "one_direction", "duplicated"])
def test_mixed_batch_in_three_spellings(mixed, how):
    from gnf_amd.graph_stats import graph_stats
    g = _spell(mixed["graphs"], how, np.random.default_rng(7))
    got = _host(graph_stats(g))
    assert got["degree_hist"].shape == (9, 130) and got["clustering_hist"].shape == (9, 100)
    _assert_stats(got, mixed["want"], how)
    # the sizes given on the host (nothing is read back before the launch): same result
    _assert_stats(_host(graph_stats(g, n_node_host=mixed["n_node"])), mixed["want"], how + ", n_node_host")


def test_more_neighbours_than_a_workgroup_has_lanes():
    from gnf_amd.graph_stats import graph_stats
    n = 340
    s, r = R.complete(n)
    got = _host(graph_stats(_graph([n], [len(s)], s, r)))
    assert (got["degree"] == n - 1).all() and (got["triangles"] == 57291).all()
    assert got["degree_hist"][0, n - 1] == n and got["degree_hist"].sum() == n
    assert got["clustering_hist"][0, 99] == n and got["clustering_hist"].sum() == n
    assert got["n_edges"].tolist() == [math.comb(n, 2)] and got["n_triangles"].tolist() == [math.comb(n, 3)]
    assert (got["clustering"] == 1.0).all()


def test_a_hub_whose_neighbours_drain_the_queue_twice_with_a_remainder():
    """The 131-node star with six extra edges next to K70: the hub's 130 neighbours pass through the 128-entry queue as 64 + 64 +
    2 and its row spans three words that are almost empty in every other row; against the host reference and against the
    degree and triangle columns of graph_orbits, which shares the walk."""
    import graph_orbits_ref as OR
    from gnf_amd.graph_stats import graph_orbits, graph_stats
    graphs = [(131, OR.big_star()), (70, R.complete(70))]
    g = _spell(graphs, "one_direction", None)
    n_node, s, r = R.batch(graphs)
    want = R.graph_stats(n_node, s, r)
    assert want["degree"][0] == 130 and want["triangles"][0] == 6 and want["n_triangles"].tolist() == [6, math.comb(70, 3)]
    got = _host(graph_stats(g))
    _assert_stats(got, want)
    orbits = graph_orbits(g)["orbits"].cpu().numpy()
    np.testing.assert_array_equal(got["degree"], orbits[:, 0])
    np.testing.assert_array_equal(got["triangles"], orbits[:, 3])


def test_decoded_graph_needs_no_csr_build(decoded, monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.graph_stats import graph_stats

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR decode_graphs seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    got = _host(graph_stats(decoded["graph"]))
    _assert_stats(got, decoded["want"])
    assert got["n_triangles"].sum() > 1000 and got["clustering_hist"][:, 99].sum() > 100    # cliques


def test_a_wider_bound_pads_the_degree_histogram(mixed):
    from gnf_amd.graph_stats import graph_stats
    g = _spell(mixed["graphs"], "one_direction", None)
    got = _host(graph_stats(g, max_nodes_per_graph=200, clustering_bins=7))
    want = R.graph_stats(mixed["n_node"], g.senders.cpu().numpy(), g.receivers.cpu().numpy(), max_nodes=200, bins=7)
    assert got["degree_hist"].shape == (9, 200) and got["clustering_hist"].shape == (9, 7)
    np.testing.assert_array_equal(got["degree_hist"][:, :130], mixed["want"]["degree_hist"])
    assert got["degree_hist"][:, 130:].sum() == 0
    _assert_stats(got, want, "max_nodes_per_graph=200, 7 bins")
    with pytest.raises(ValueError):
        graph_stats(g, n_node_host=mixed["n_node"], max_nodes_per_graph=129)


# ---- 2. hist_mmd -----------------------------------------------------------------------------------------------------------
def _hists(rng, rows, width, zero_row):
    h = rng.integers(0, 20, size=(rows, width)).astype(np.int32)
    h[:, 0] += 1                      # (no row all-zero by accident, one column included)
    h[zero_row] = 0
    return h


@pytest.mark.parametrize("la,lb", [(1, 63), (63, 64), (64, 65), (65, 130), (130, 1), (64, 64)])
def test_hist_mmd_against_float64(la, lb):
    from gnf_amd.graph_stats import _hist_mmd_sums, hist_mmd
    rng = np.random.default_rng(1000 * la + lb)
    ha, hb = _hists(rng, 7, la, 3), _hists(rng, 5, lb, 4)
    ta, tb = torch.as_tensor(ha).to(DEV), torch.as_tensor(hb).to(DEV)
    for kernel in ("gaussian_emd", "gaussian_tv"):
        for sigma, scale in ((1.0, 1.0), (0.1, 100.0)):
            want = R.mmd2(ha, hb, kernel, sigma, scale)
            got = hist_mmd(ta, tb, kernel, sigma, scale)
            assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == "cuda"
            err = abs(float(got) - want)
            print(f"La={la} Lb={lb} {kernel} sigma={sigma} scaling={scale}: MMD^2 {float(got):.17g} vs {want:.17g}, |err| {err:.3g}")
            assert err <= MMD_ATOL
            sums = _hist_mmd_sums(ta, tb, kernel, sigma, scale)
            ref = R.mmd_sums(ha, hb, kernel, sigma, scale)
            assert sums[3:].tolist() == [6.0, 4.0] == ref[3:].tolist()
            np.testing.assert_allclose(sums.cpu().numpy()[:3], ref[:3], rtol=0, atol=1e-10)
            # bit-reproducible
            assert torch.equal(_hist_mmd_sums(ta, tb, kernel, sigma, scale), sums)
            assert torch.equal(hist_mmd(ta, tb, kernel, sigma, scale), got)


def test_hist_mmd_single_rows_and_empty_sets():
    from gnf_amd.graph_stats import hist_mmd
    a, b = torch.tensor([[1, 0]], dtype=torch.int32, device=DEV), torch.tensor([[0, 3]], dtype=torch.int32, device=DEV)
    assert abs(float(hist_mmd(a, b)) - (2.0 - 2.0 * math.exp(-0.5))) <= MMD_ATOL
    assert abs(float(hist_mmd(a, b, "gaussian_tv", 0.5)) - (2.0 - 2.0 * math.exp(-2.0))) <= MMD_ATOL
    assert abs(float(hist_mmd(a, 5 * a))) <= MMD_ATOL
    rng = np.random.default_rng(5)
    ha, hb = rng.integers(0, 9, size=(1, 130)).astype(np.int32), rng.integers(0, 9, size=(1, 65)).astype(np.int32)
    got = float(hist_mmd(torch.as_tensor(ha).to(DEV), torch.as_tensor(hb).to(DEV), sigma=3.0))
    assert abs(got - R.mmd2(ha, hb, sigma=3.0)) <= MMD_ATOL
    with pytest.raises(ValueError):
        hist_mmd(torch.zeros(2, 4, dtype=torch.int32, device=DEV), b)
    with pytest.raises(ValueError):
        hist_mmd(a, torch.zeros(0, 2, dtype=torch.int32, device=DEV))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
def test_evaluate_generated(mixed, decoded):
    from gnf_amd.graph_stats import evaluate_generated, graph_stats
    g = _spell(mixed["graphs"], "both_loops_shuffled", np.random.default_rng(8))
    want = R.evaluate(mixed["want"], decoded["want"])
    assert want["degree_mmd"] > 1e-3 and want["clustering_mmd"] > 1e-3
    from_stats = evaluate_generated(graph_stats(g), graph_stats(decoded["graph"]))
    from_graphs = evaluate_generated(g, decoded["graph"])
    for k in ("degree_mmd", "clustering_mmd"):
        print(f"{k}: {float(from_stats[k]):.17g} vs {want[k]:.17g}")
        assert from_stats[k].dtype == torch.float64 and from_stats[k].dim() == 0
        assert abs(float(from_stats[k]) - want[k]) <= MMD_ATOL
        assert torch.equal(from_graphs[k], from_stats[k])
    same = evaluate_generated(g, g)
    assert abs(float(same["degree_mmd"])) <= MMD_ATOL and abs(float(same["clustering_mmd"])) <= MMD_ATOL
