"""gnf_amd.graph_stats.graph_orbits / orbit_mmd (gnf_graph_orbits, gnf_vec_mmd_i64) on the MI355X against the brute-force
enumeration of tests/graph_orbits_ref.py.

Integer outputs (orbits, orbit_sums) are asserted EQUAL - nothing is excluded; orbit_mean is their fp64 quotient, one IEEE
division on both sides, asserted equal too.  The MMD block sums are held to an absolute error of 1e-10 against the float64
reference, the tolerance test_hist_mmd_against_float64 uses for the same reduction shape: a kernel value k = exp(-u) in
[0, 1] carries the relative error of u (15 squares added in another order, about 15 * 2^-53) damped by u e^-u <= 1 / e, far
below 1e-13 per pair, and a block sum adds at most 81 of them.  The reduction is bit-reproducible, and two identical sets
give exactly 0."""
import math

import numpy as np
import pytest
import torch

import decode_graphs_ref as DR
import graph_orbits_ref as R
import graph_stats_ref as S
from helpers import graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MMD_ATOL = 1e-10
SPELLINGS = ["symmetric", "one_direction", "duplicates_and_loops"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _graph(n_node, n_edge, s, r):
    return graph_from_arrays(n_node, n_edge, s, r, np.zeros((int(np.sum(n_node)), 1), np.float32), DEV)


def _spell(graphs, how, rng):
    """One GraphsTuple spelling of [(n, (s, r) local, one direction)]: edges stay grouped by graph (the block-diagonal layout)."""
    n_node, n_edge, ss, rr, off = [], [], [], [], 0
    for n, (s, r) in graphs:
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
    return _graph(n_node, n_edge, np.concatenate(ss), np.concatenate(rr))


def _host(out):
    assert set(out) >= {"orbits", "orbit_sums", "orbit_mean"}
    assert out["orbits"].dtype == torch.int64 and out["orbit_sums"].dtype == torch.int64
    assert out["orbit_mean"].dtype == torch.float64 and all(v.device.type == "cuda" for v in out.values())
    assert out["orbits"].shape[1:] == (15,) and out["orbit_sums"].shape[1:] == (15,) == out["orbit_mean"].shape[1:]
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_orbits(got, want, what=""):
    np.testing.assert_array_equal(got["orbits"], want["orbits"], err_msg=f"orbits {what}")
    np.testing.assert_array_equal(got["orbit_sums"], want["orbit_sums"], err_msg=f"orbit_sums {what}")
    np.testing.assert_array_equal(got["orbit_mean"], want["orbit_mean"], err_msg=f"orbit_mean {what}")


@pytest.fixture(scope="module")
def mixed():
    """Graphs of 0 .. 3 nodes, the pinned graphs of the definition and G(40, 0.3); after the first graph no graph starts on a
    multiple of 64 rows."""
    rng = np.random.default_rng(20241)
    graphs = [(3, S.complete(3)), (0, S.complete(0)), (1, S.complete(1)), (2, S.complete(2)), (5, S.complete(5)),
              (4, S.cycle(4)), (7, S.cycle(7)), (10, R.petersen()), (6, R.complete_bipartite(3, 3)), (4, R.tailed_triangle()),
              (4, R.chorded_cycle()), (40, S.gnp(40, 0.3, rng)), (7, S.star(7)), (3, S.cycle(3))]
    n_node, s, r = S.batch(graphs)
    assert all(o % 64 for o in np.cumsum(n_node)[:-1])
    want = R.graph_orbits(n_node, s, r)
    assert want["orbits"][3 + 1 + 2].tolist() == [4, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4]          # K5
    assert (want["orbit_sums"][11] > 0).all()                                                            # G(40, 0.3): every orbit
    return {"graphs": graphs, "n_node": n_node, "want": want}


@pytest.fixture(scope="module")
def mixed_orbits(mixed):
    """graph_orbits of the mixed batch (symmetric spelling), computed once for the tests that only read it"""
    from gnf_amd.graph_stats import graph_orbits
    g = _spell(mixed["graphs"], "symmetric", None)
    return g, graph_orbits(g)


# ---- 1. integer outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", SPELLINGS)
def test_mixed_batch_in_three_spellings(mixed, how):
    from gnf_amd.graph_stats import graph_orbits
    g = _spell(mixed["graphs"], how, np.random.default_rng(7))
    first = graph_orbits(g)
    got = _host(first)
    assert got["orbits"].shape == (sum(mixed["n_node"]), 15) and got["orbit_sums"].shape == (len(mixed["n_node"]), 15)
    _assert_orbits(got, mixed["want"], how)
    # the sizes given on the host (nothing is read back before the launch): same result, and the same bits twice
    again = graph_orbits(g, n_node_host=mixed["n_node"])
    for k in ("orbits", "orbit_sums", "orbit_mean"):
        assert torch.equal(again[k], first[k]), k


def _boundary_positions(n):
    """20 local indices of an n-node graph straddling 63 / 64 and 127 / 128 as far as the graph reaches"""
    pos = [p for p in list(range(58, 68)) + list(range(119, 129)) if p < n]
    fill = 57
    while len(pos) < 20:
        pos.append(fill)
        fill -= 1
    return sorted(pos)


def test_word_boundaries_and_a_wider_bound():
    from gnf_amd.graph_stats import graph_orbits
    rng = np.random.default_rng(64)
    graphs, rows = [], []
    for n in (64, 65, 128, 129):
        pos = np.asarray(_boundary_positions(n))
        assert len(set(pos.tolist())) == 20 and pos.max() == min(n - 1, 128) and pos.min() <= 63
        s, r = S.gnp(20, 0.4, rng)
        sub = R.node_orbits(S.dense_adjacency(20, s, r))
        assert sub[:, 14].sum() > 0 and sub[:, 8].sum() > 0
        full = np.zeros((n, 15), np.int64)            # every other node is isolated: all-zero rows
        full[pos] = sub
        rows.append(full)
        graphs.append((n, (pos[s], pos[r])))
    want = np.concatenate(rows)
    sums = np.stack([f.sum(0) for f in rows])
    g = _spell(graphs, "one_direction", None)
    tight = graph_orbits(g)
    np.testing.assert_array_equal(tight["orbits"].cpu().numpy(), want)
    np.testing.assert_array_equal(tight["orbit_sums"].cpu().numpy(), sums)
    for cap in (130, 200):   # a bound above the largest graph: 3 and 4 words per row where 3 are used
        wide = graph_orbits(g, max_nodes_per_graph=cap)
        for k in ("orbits", "orbit_sums", "orbit_mean"):
            assert torch.equal(wide[k], tight[k]), (k, cap)
    with pytest.raises(ValueError):
        graph_orbits(g, n_node_host=[64, 65, 128, 129], max_nodes_per_graph=128)
    with pytest.raises(ValueError):
        graph_orbits(g, max_nodes_per_graph=8193)


@pytest.fixture(scope="module")
def big_star_want():
    """brute force on the 131-node star with six extra edges: a few seconds, once"""
    return R.node_orbits(S.dense_adjacency(131, *R.big_star()))


def test_more_neighbours_than_the_queue_holds(big_star_want):
    from gnf_amd.graph_stats import graph_orbits
    hub = [0] * 15
    hub[0], hub[2], hub[3], hub[7], hub[11], hub[13] = 130, 8379, 6, 356995, 762, 3
    assert big_star_want[0].tolist() == hub
    n = 70
    g = _spell([(131, R.big_star()), (n, S.complete(n))], "one_direction", None)
    got = _host(graph_orbits(g))
    np.testing.assert_array_equal(got["orbits"][:131], big_star_want)
    assert got["orbits"][0].tolist() == hub
    k70 = [0] * 15
    k70[0], k70[3], k70[14] = n - 1, math.comb(n - 1, 2), math.comb(n - 1, 3)
    assert got["orbits"][131:].tolist() == [k70] * n
    assert got["orbit_sums"].tolist() == [big_star_want.sum(0).tolist(), [n * v for v in k70]]


# ---- 2. ties to what exists ------------------------------------------------------------------------------------------------
def test_degree_and_triangles_match_graph_stats(mixed, mixed_orbits, community_medium):
    from gnf_amd.graph_stats import graph_orbits, graph_stats
    from oracle import gnf_oracle as O
    g, orb = mixed_orbits
    st = graph_stats(g)
    assert torch.equal(orb["orbits"][:, 0], st["degree"].to(torch.int64))
    assert torch.equal(orb["orbits"][:, 3], st["triangles"].to(torch.int64))
    nn, ne, s, r = O.batch_graphs(*community_medium, [5])
    cm = graph_from_arrays(nn, ne, s, r, np.zeros((int(nn.sum()), 1), np.float32), DEV)
    orb, st = graph_orbits(cm), graph_stats(cm)
    assert int(st["n_triangles"].sum()) > 0
    assert torch.equal(orb["orbits"][:, 0], st["degree"].to(torch.int64))
    assert torch.equal(orb["orbits"][:, 3], st["triangles"].to(torch.int64))
    assert orb["orbit_sums"][0, 0].item() == 2 * st["n_edges"][0].item()
    assert orb["orbit_sums"][0, 3].item() == 3 * st["n_triangles"][0].item()


def test_decoded_graph_needs_no_csr_build(monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs
    from gnf_amd.graph_stats import graph_orbits
    n_node = [1, 12, 0, 33, 20]
    z, _ = DR.clustered_embeddings(np.random.default_rng(3), n_node, 3)
    shell = graph_from_arrays(n_node, np.zeros(len(n_node), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)
    graph = decode_graphs(shell, self_loops=True)["graph"]
    s, r = graph.senders.cpu().numpy(), graph.receivers.cpu().numpy()
    assert len(s) > sum(n_node)
    want = R.graph_orbits(n_node, s, r)
    assert want["orbit_sums"][:, 14].sum() > 100    # cliques

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR decode_graphs seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    _assert_orbits(_host(graph_orbits(graph)), want)


# ---- 3. orbit_mmd ----------------------------------------------------------------------------------------------------------
def _pair(want, ids):
    """(orbit_sums, n_node) device pair of some graphs of a reference result, and the same on the host"""
    sums = want["orbit_sums"][ids]
    cnt = np.asarray(want["n_node"], np.int32)[ids]
    return (torch.as_tensor(sums).to(DEV), torch.as_tensor(cnt).to(DEV)), (sums, cnt)


@pytest.mark.parametrize("ids_a,ids_b", [([5], list(range(9))), (list(range(9)), [2, 3, 9, 12, 13]),
                                          ([1, 4, 8, 10, 11], [6]), (list(range(14)), list(range(14)))],
                         ids=["1x9", "9x5", "5x1", "14x14"])
def test_orbit_mmd_against_float64(mixed, ids_a, ids_b):
    from gnf_amd.graph_stats import _orbit_mmd_sums, orbit_mmd
    want = dict(mixed["want"], n_node=mixed["n_node"])
    (da, ha), (db, hb) = _pair(want, ids_a), _pair(want, ids_b)
    for sigma in (30.0, 4.0):
        ref = R.vec_mmd_sums(ha[0], ha[1], hb[0], hb[1], sigma)
        sums = _orbit_mmd_sums(da, db, sigma)
        host = sums.cpu().numpy()
        print(f"sigma={sigma}: sums {host.tolist()} vs {ref.tolist()}, |err| {np.abs(host - ref).max():.3g}")
        assert host[3:].tolist() == ref[3:].tolist() == [float(sum(1 for i in ids if mixed["n_node"][i] > 0))
                                                         for ids in (ids_a, ids_b)]
        np.testing.assert_allclose(host[:3], ref[:3], rtol=0, atol=MMD_ATOL)
        got = orbit_mmd(da, db, sigma)
        assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == "cuda"
        assert abs(float(got) - R.vec_mmd2(ha[0], ha[1], hb[0], hb[1], sigma)) <= MMD_ATOL
        # bit-reproducible
        assert torch.equal(_orbit_mmd_sums(da, db, sigma), sums) and torch.equal(orbit_mmd(da, db, sigma), got)
        if ids_a == ids_b:
            assert float(got) == 0.0 and host[0] == host[1] == host[2]
        else:
            assert float(got) > 1e-3


def test_orbit_mmd_of_results_single_rows_and_empty_sets(mixed, mixed_orbits):
    from gnf_amd.graph_stats import orbit_mmd
    _, orb = mixed_orbits
    assert float(orbit_mmd(orb, orb)) == 0.0                                         # two results of graph_orbits
    pair = (orb["orbit_sums"], orb["n_node"])
    assert float(orbit_mmd(orb, pair)) == 0.0 and float(orbit_mmd(pair, orb, 4.0)) == 0.0
    a = (torch.tensor([[30, 0, 12]], device=DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    b = (torch.tensor([[0, 40, 12]], device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV))
    d2 = 15.0 ** 2 + 10.0 ** 2 + 3.0 ** 2
    assert abs(float(orbit_mmd(a, b)) - (2.0 - 2.0 * math.exp(-d2 / 1800.0))) <= MMD_ATOL
    assert abs(float(orbit_mmd(a, b, sigma=5.0)) - (2.0 - 2.0 * math.exp(-d2 / 50.0))) <= MMD_ATOL
    empty = (torch.zeros(2, 3, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    none = (torch.zeros(0, 3, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    for x, y in ((empty, b), (a, empty), (a, none), (none, none)):
        with pytest.raises(ValueError):
            orbit_mmd(x, y)


def test_evaluate_generated_with_orbits(mixed, mixed_orbits):
    from gnf_amd.graph_stats import evaluate_generated, graph_orbits, graph_stats, orbit_mmd
    g, orb = mixed_orbits
    rng = np.random.default_rng(9)
    other = [(12, S.gnp(12, 0.5, rng)), (0, S.complete(0)), (9, S.cycle(9)), (15, S.gnp(15, 0.3, rng)), (6, S.complete(6))]
    n_node, s, r = S.batch(other)
    h = _spell(other, "duplicates_and_loops", rng)
    want = R.vec_mmd2(mixed["want"]["orbit_sums"], mixed["n_node"], R.graph_orbits(n_node, s, r)["orbit_sums"], n_node, 30.0)
    plain = evaluate_generated(g, h)
    assert set(plain) == {"degree_mmd", "clustering_mmd"}
    full = evaluate_generated(g, h, True)                                # the added argument also works positionally
    assert set(full) == {"degree_mmd", "clustering_mmd", "orbit_mmd"} == set(evaluate_generated(g, h, orbits=True))
    assert torch.equal(full["degree_mmd"], plain["degree_mmd"]) and torch.equal(full["clustering_mmd"], plain["clustering_mmd"])
    print(f"orbit_mmd: {float(full['orbit_mmd']):.17g} vs {want:.17g}")
    assert full["orbit_mmd"].dtype == torch.float64 and full["orbit_mmd"].dim() == 0
    assert want > 1e-3 and abs(float(full["orbit_mmd"]) - want) <= MMD_ATOL
    assert torch.equal(full["orbit_mmd"], orbit_mmd(orb, graph_orbits(h)))
    from_dicts = evaluate_generated({**graph_stats(g), **orb}, {**graph_stats(h), **graph_orbits(h)}, orbits=True)
    assert torch.equal(from_dicts["orbit_mmd"], full["orbit_mmd"])
    with pytest.raises(ValueError):
        evaluate_generated(graph_stats(g), graph_stats(h), orbits=True)
    assert float(evaluate_generated(g, g, orbits=True)["orbit_mmd"]) == 0.0


# ---- 4. capture ------------------------------------------------------------------------------------------------------------
def test_graph_orbits_replays_bitwise(mixed, mixed_orbits):
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured with
    torch.cuda.graph as tests/test_graph_capture_gpu.py captures the flow, replayed, and compared with the eager call."""
    from gnf_amd.graph_stats import graph_orbits
    g, _ = mixed_orbits
    eager = graph_orbits(g, max_nodes_per_graph=64)          # (also the first launches: CSR and offsets caches)
    _assert_orbits(_host(eager), mixed["want"])
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = graph_orbits(g, max_nodes_per_graph=64)
    for _ in range(2):
        captured["orbits"].zero_(), captured["orbit_sums"].fill_(7), captured["orbit_mean"].zero_()
        cg.replay()
        torch.cuda.synchronize()
        for k in ("orbits", "orbit_sums", "orbit_mean"):
            assert torch.equal(captured[k], eager[k]), k
