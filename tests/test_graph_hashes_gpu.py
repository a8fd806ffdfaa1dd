"""gnf_amd.graph_stats.graph_hashes / uniqueness_novelty (gnf_graph_hashes, gnf_graph_hash_match) on the MI355X against the numpy
uint64 reference of tests/graph_hashes_ref.py (itself checked against a second construction and against hand-computed values in
tests/test_graph_hashes_cpu.py).

Every output is an integer with one definition (include/gnf_graph_hashes.h), so every comparison is for EQUALITY, bit for bit;
there is no tolerance anywhere in this file.  The cases are the smallest that reach each mistake a kernel can make: duplicates
counted twice and the diagonal counted as an edge (the spellings), neighbours beyond the first bitmap word (the edge 63 - 64,
K65), the last partial word (the hub in column 69), the graph's offset inside a batch (an empty graph between two others), the
round salt and the colour double buffer (rounds 2 and up on irregular graphs), and the switch between the LDS and the global
route (the same batch on both sides of WL_LDS_NODES, a graph of exactly that size, graphs above it)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_graphs_ref as DR
import graph_components_ref as CR
import graph_hashes_ref as R
import graph_stats_ref as S
from helpers import graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPELLINGS = ["symmetric", "one_direction", "duplicates_and_loops"]
ROUNDS = [0, 1, 2, 3, 64]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _graph(spelled):
    n_node, n_edge, s, r = spelled
    return graph_from_arrays(n_node, n_edge, s, r, np.zeros((int(np.sum(n_node)), 1), np.float32), DEV)


@pytest.fixture(scope="module")
def small():
    """the small cases, their flat batch and the reference per round count - computed once, never edited"""
    cases = R.small_cases()
    n_node, _, s, r = R.spell(cases, "one_direction")
    return {"cases": cases, "flat": (n_node, s, r), "want": {it: R.hashes(n_node, s, r, it) for it in ROUNDS}}


def _assert_hashes(out, want, what=""):
    from gnf_amd.graph_stats import HASH_KEYS
    assert tuple(out) == HASH_KEYS == R.KEYS
    for k in R.KEYS:
        assert out[k].dtype == (torch.int32 if k == "n_node" else torch.int64) and out[k].device.type == "cuda", k
        np.testing.assert_array_equal(out[k].cpu().numpy(), want[k], err_msg=f"{what} {k}")


# ---- 1. the hash: every case, every spelling, every round count, both routes ----------------------------------------------
@pytest.mark.parametrize("how", SPELLINGS)
def test_small_cases_equal_the_reference(small, how):
    from gnf_amd.graph_stats import WL_LDS_NODES, graph_hashes
    g = _graph(R.spell(small["cases"], how, np.random.default_rng(7)))
    for it in ROUNDS:
        out = graph_hashes(g, iterations=it)                                      # LDS route, 130 columns
        print(how, it, [hex(v & (2 ** 64 - 1)) for v in out["hash"].cpu().tolist()[:4]])
        _assert_hashes(out, small["want"][it], f"{how} rounds={it}")
        again = graph_hashes(g, iterations=it)                                    # two calls give the same bits
        assert all(torch.equal(again[k], out[k]) for k in R.KEYS)
        other = graph_hashes(g, iterations=it, max_nodes_per_graph=WL_LDS_NODES + 1)      # the global route
        _assert_hashes(other, small["want"][it], f"{how} rounds={it} global route")
    wide = graph_hashes(g, max_nodes_per_graph=300)                               # the 1024-thread workgroup of the LDS route
    _assert_hashes(wide, small["want"][3], f"{how} bound 300")


def test_small_cases_are_what_they_claim(small):
    at = {c[0]: k for k, c in enumerate(small["cases"])}
    w = small["want"]
    assert [n for _, n, _ in small["cases"]][:3] == [3, 0, 1]                      # an empty graph between two others
    for it in ROUNDS:
        h = w[it]["hash"]
        assert h[at["path130"]] == h[at["path130_reversed"]] == h[at["path130_folded"]]
        assert len(set(h.tolist())) == len(small["cases"]) - 2
    assert w[3]["n_edges"][at["edge_63_64"]] == 1 and w[3]["n_edges"][at["K65"]] == 65 * 64 // 2
    for name in ("sparse40", "sparse129"):        # irregular: from round 2 on a mixed-up colour buffer or salt shows
        k = at[name]
        assert len({w[it]["hash"][k] for it in ROUNDS}) == len(ROUNDS)
        a = int(np.sum([n for _, n, _ in small["cases"]][:k]))
        n = small["cases"][k][1]
        colours = [len(set(w[it]["node_colour"][a:a + n].tolist())) for it in (0, 1, 2)]
        assert colours[0] < colours[1] < colours[2], (name, colours)


def test_labels_and_the_same_labels_permuted(small):
    from gnf_amd.graph_stats import WL_LDS_NODES, graph_hashes
    rng = np.random.default_rng(12)
    n_node, s, r = small["flat"]
    n = sum(n_node)
    labels = rng.integers(-2, 3, n)
    want = R.hashes(n_node, s, r, 3, labels)
    assert (want["hash"] != small["want"][3]["hash"])[np.array(n_node) > 1].all()
    g = _graph(R.spell(small["cases"], "symmetric"))
    lab = torch.as_tensor(labels).to(DEV)
    for kw in ({}, {"max_nodes_per_graph": WL_LDS_NODES + 1}):
        _assert_hashes(graph_hashes(g, labels=lab, **kw), want, f"labels {kw}")
    # every graph renumbered by a permutation of its own, labels moved alike: the same hashes, the colours moved alike
    moved_cases, moved_labels, perms, off = [], np.zeros(n, np.int64), [], 0
    for name, k, edges in small["cases"]:
        p = rng.permutation(k)
        moved_cases.append((name, k, R.permuted(k, edges, p)))
        moved_labels[off + p] = labels[off:off + k]
        perms.append(off + p)
        off += k
    out = graph_hashes(_graph(R.spell(moved_cases, "one_direction")), labels=torch.as_tensor(moved_labels).to(DEV))
    np.testing.assert_array_equal(out["hash"].cpu().numpy(), want["hash"])
    np.testing.assert_array_equal(out["node_colour"].cpu().numpy()[np.concatenate(perms)], want["node_colour"])
    with pytest.raises(ValueError):
        graph_hashes(g, labels=lab[:-1])
    with pytest.raises(ValueError):
        graph_hashes(g, labels=lab.to(torch.int32))
    with pytest.raises(ValueError):
        graph_hashes(g, iterations=65)


# ---- 2. the route boundary -------------------------------------------------------------------------------------------------
def test_one_batch_on_both_sides_of_the_route_bound():
    """a graph of exactly WL_LDS_NODES nodes (all 64 KiB of colours in LDS, 64 words per row) between two small ones: the default
    bound and max_nodes_per_graph = WL_LDS_NODES take the LDS route, WL_LDS_NODES + 1 the global route"""
    from gnf_amd.graph_stats import WL_LDS_NODES, graph_hashes
    rng = np.random.default_rng(4096)
    cases = [("sparse129", 129, CR.sparse(129, rng, 2.5)), ("lattice", WL_LDS_NODES, CR.stride_lattice(WL_LDS_NODES, rng)),
             ("K3", 3, S.complete(3)), ("sparse300", 300, CR.sparse(300, rng, 2.5))]      # 300: irregular, rows of five words
    n_node, _, s, r = R.spell(cases, "one_direction")
    g = _graph(R.spell(cases, "symmetric"))
    for it in (2, 3):
        want = R.hashes(n_node, s, r, it)
        assert len(set(want["node_colour"][129:129 + WL_LDS_NODES].tolist())) > 20        # (something to refine)
        outs = [graph_hashes(g, iterations=it, **kw)
                for kw in ({}, {"max_nodes_per_graph": WL_LDS_NODES}, {"max_nodes_per_graph": WL_LDS_NODES + 1})]
        for out in outs:
            _assert_hashes(out, want, f"rounds={it}")
        for k in ("hash", "node_colour"):
            assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), k


def test_graphs_above_the_route_bound():
    """4 200 and 16 500 nodes (graph_components_ref.large_cases): real graphs on the global route, rows of more than 64 words"""
    from gnf_amd.graph_stats import WL_LDS_NODES, graph_hashes
    assert WL_LDS_NODES < 4200
    cases = CR.large_cases()
    n_node, _, s, r = R.spell(cases, "one_direction")
    want = R.hashes(n_node, s, r, 3)
    g = _graph(R.spell(cases, "one_direction"))
    _assert_hashes(graph_hashes(g), want, "large")
    _assert_hashes(graph_hashes(g, max_nodes_per_graph=65536, n_node_host=n_node), want, "large, bound 65536")


def test_graphs_without_nodes_and_an_empty_batch():
    from gnf_amd.graph_stats import graph_hashes, uniqueness_novelty
    for sizes in ([0, 0, 0], []):
        g = graph_from_arrays(sizes, [0] * len(sizes), [], [], np.zeros((0, 2), np.float32), DEV)
        for it in (0, 2):
            _assert_hashes(graph_hashes(g, iterations=it), R.hashes(sizes, [], [], it), str(sizes))
        with pytest.raises(ValueError):
            uniqueness_novelty(g, g)                                  # no generated graph has a node


# ---- 3. capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "global"])
def test_graph_hashes_replays_on_a_second_batch_in_the_same_buffers(small, route):
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured on CSR buffers that
    hold the first batch, the second batch (same sizes, every graph mirrored, other edges in the sparse graphs' place) is copied
    into those buffers, and the replay equals the eager call on the second batch."""
    from gnf_amd.graphs import Csr, csr_of, seed_csr_cache
    from gnf_amd.graph_stats import WL_LDS_NODES, graph_hashes
    cap = 200 if route == "lds" else WL_LDS_NODES + 1
    cases = small["cases"]
    rng = np.random.default_rng(3)
    twin = []
    for name, n, (s, r) in cases:
        if name.startswith("sparse"):       # as many edges, drawn anew
            i, j = np.triu_indices(n, 1)
            pick = rng.choice(len(i), size=len(s), replace=False)
            twin.append((name, n, (i[pick], j[pick])))
        else:
            twin.append((name, n, (n - 1 - np.asarray(s, np.int64), n - 1 - np.asarray(r, np.int64))))
    first, second = _graph(R.spell(cases, "symmetric")), _graph(R.spell(twin, "symmetric"))
    n_node, _, s2, r2 = R.spell(twin, "one_direction")
    want_second = R.hashes(n_node, s2, r2, 3)
    assert (want_second["hash"] != small["want"][3]["hash"]).any()
    eager = [graph_hashes(g, max_nodes_per_graph=cap) for g in (first, second)]
    _assert_hashes(eager[0], small["want"][3], "first")
    _assert_hashes(eager[1], want_second, "second")
    ca, cb = csr_of(first), csr_of(second)
    assert ca.n_edges == cb.n_edges
    rowptr, col = ca.rowptr.clone(), ca.col.clone()
    held = first.replace(senders=first.senders.clone(), receivers=first.receivers.clone())     # a key of its own in the cache
    seed_csr_cache(held, Csr(rowptr, col, ca.n_nodes, ca.n_edges))
    warm = graph_hashes(held, max_nodes_per_graph=cap)              # (also the offsets cache of this n_node tensor)
    assert all(torch.equal(warm[k], eager[0][k]) for k in R.KEYS)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = graph_hashes(held, max_nodes_per_graph=cap)
    for src, want in ((cb, eager[1]), (ca, eager[0]), (cb, eager[1])):
        rowptr.copy_(src.rowptr), col.copy_(src.col)
        for k in R.KEYS[:3]:
            captured[k].fill_(77)
        cg.replay()
        torch.cuda.synchronize()
        for k in R.KEYS:
            assert torch.equal(captured[k], want[k]), k


# ---- 4. data and pipeline --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    """grid_small whole and the first 32 graphs of citeseer_small, with their reference hashes"""
    out = {}
    for name, index in (("grid_small", None), ("citeseer_small", range(32))):
        spelled = R.dataset(name, index)
        out[name] = (spelled, R.hashes(spelled[0], spelled[2], spelled[3], 3))
    return out


@pytest.mark.parametrize("name", ["grid_small", "citeseer_small"])
def test_data_sets_equal_the_reference(data, name):
    from gnf_amd.graph_stats import graph_hashes
    spelled, want = data[name]
    _assert_hashes(graph_hashes(_graph(spelled)), want, name)


def _assert_shares(out, m, what=""):
    from gnf_amd.graph_stats import NOVELTY_KEYS
    assert tuple(out) == NOVELTY_KEYS
    for k in ("first_in_generated", "match_in_training", "counts"):
        assert out[k].dtype == (torch.int64 if k == "counts" else torch.int32) and out[k].device.type == "cuda"
        np.testing.assert_array_equal(out[k].cpu().numpy(), m[k], err_msg=f"{what} {k}")
    for k, v in R.shares(m).items():
        assert out[k].dtype == torch.float64 and out[k].dim() == 0 and out[k].device.type == "cuda"
        assert float(out[k]) == v, (what, k)      # the quotient of two small integers in float64, formed the same way


def test_uniqueness_and_novelty_equal_the_reference(data):
    from gnf_amd.graph_stats import graph_hashes, uniqueness_novelty
    (nn, ne, s, r), train = data["citeseer_small"]
    tg = _graph((nn, ne, s, r))
    # generated = training: nothing is novel, uniqueness = classes / graphs
    m = R.match(train["hash"], nn, train["hash"], nn)
    classes = len(set(zip(train["hash"].tolist(), nn)))
    assert m["counts"].tolist() == [32, classes, 0, 0] and classes < 32
    _assert_shares(uniqueness_novelty(tg, tg), m, "generated = training")
    hashed = graph_hashes(tg)
    _assert_shares(uniqueness_novelty(hashed, hashed), m, "hashes passed in")
    # generated = some training graphs renumbered (one of them twice), an empty graph, and two graphs the training set lacks
    rng = np.random.default_rng(21)
    off = np.concatenate([[0], np.cumsum(nn)])
    picked = [5, 17, 5, 30]
    cases = []
    for g in picked:
        sel = (s >= off[g]) & (s < off[g + 1])
        cases.append((f"train{g}", nn[g], R.permuted(nn[g], (s[sel] - off[g], r[sel] - off[g]), rng.permutation(nn[g]))))
    cases[2:2] = [("empty", 0, CR.no_edges(0)), ("K7", 7, S.complete(7))]
    cases.append(("path23", 23, CR.path(23)))
    gn, ge, gs, gr = R.spell(cases, "one_direction")
    gen = R.hashes(gn, gs, gr, 3)
    m = R.match(gen["hash"], gn, train["hash"], nn)
    assert m["match_in_training"][[2, 3, 6]].tolist() == [-1, -1, -1] and (m["match_in_training"][[0, 1, 4, 5]] >= 0).all()
    assert m["match_in_training"][0] <= 5 and m["first_in_generated"].tolist() == [0, 1, -1, 3, 0, 5, 6]
    assert m["counts"].tolist() == [6, 5, 2, 2]
    _assert_shares(uniqueness_novelty(_graph((gn, ge, gs, gr)), hashed), m, "renumbered copies and two new graphs")
    # an empty training set: everything valid is novel
    none = {"hash": hashed["hash"][:0], "n_node": hashed["n_node"][:0]}
    _assert_shares(uniqueness_novelty(_graph((gn, ge, gs, gr)), none), R.match(gen["hash"], gn, gen["hash"][:0], []), "b = 0")


def test_evaluate_generated_with_a_training_set(data):
    from gnf_amd.graph_stats import evaluate_generated, graph_hashes, keep_subgraphs, uniqueness_novelty
    (nn, ne, s, r), _ = data["grid_small"]
    train = _graph((nn, ne, s, r))
    # generated: two training graphs with one edge removed each time (what is left is new, or falls apart), one kept whole
    cases = []
    off = np.concatenate([[0], np.cumsum(nn)])
    for g, drop in ((0, 1), (3, 1), (3, None)):       # (edge 0 of a graph is a self loop)
        sel = (s >= off[g]) & (s < off[g + 1])
        ls, lr = s[sel] - off[g], r[sel] - off[g]
        keep = np.ones(len(ls), bool)
        if drop is not None:
            keep &= ~(((ls == ls[drop]) & (lr == lr[drop])) | ((ls == lr[drop]) & (lr == ls[drop])))
        cases.append((f"train{g}", nn[g], (ls[keep], lr[keep])))
    gen = _graph(R.spell(cases, "one_direction"))
    plain = evaluate_generated(gen, train)
    assert set(plain) == {"degree_mmd", "clustering_mmd"}                        # exactly today's keys
    scored = evaluate_generated(gen, train, train=train)
    assert set(scored) == set(plain) | {"uniqueness", "novelty", "unique_novel"}
    for k in plain:
        assert torch.equal(scored[k], plain[k]), k
    direct = uniqueness_novelty(gen, train)
    assert all(torch.equal(scored[k], direct[k]) for k in ("uniqueness", "novelty", "unique_novel"))
    assert float(scored["novelty"]) == 2 / 3 and float(scored["uniqueness"]) == 1.0
    # with keep= the reduced batch is what is hashed; the training hashes may be passed in
    cut = evaluate_generated(gen, train, keep="largest_component", train=graph_hashes(train), orbits=True)
    assert set(cut) == set(plain) | {"orbit_mmd", "uniqueness", "novelty", "unique_novel"}
    kept = uniqueness_novelty(keep_subgraphs(gen, "largest_component")["graph"], train)
    assert all(torch.equal(cut[k], kept[k]) for k in ("uniqueness", "novelty", "unique_novel"))


def test_decoded_graphs_are_hashed_without_building_a_csr(monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs
    from gnf_amd.graph_stats import graph_hashes, uniqueness_novelty
    n_node = [1, 12, 0, 33, 70]
    z, labels = DR.clustered_embeddings(np.random.default_rng(3), n_node, 8)
    closed = DR.edges_from_blocks(DR.clique_blocks(n_node, labels), 0.5, False)      # what the decoder must produce
    want = R.hashes(n_node, closed["senders"], closed["receivers"], 3)
    shell = graph_from_arrays(n_node, np.zeros(len(n_node), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)
    graph = decode_graphs(shell)["graph"]
    np.testing.assert_array_equal(graph.senders.cpu().numpy(), closed["senders"])

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR was seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    out = graph_hashes(graph)
    _assert_hashes(out, want, "decoded")
    shares = uniqueness_novelty(graph, out)
    assert shares["counts"].tolist() == [4, 4, 0, 0] and float(shares["novelty"]) == 0.0


# ---- 5. raw entry points ---------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched(small):
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    g = _graph(R.spell(small["cases"], "symmetric"))
    n, b = int(g.nodes.shape[0]), int(g.n_node.shape[0])
    desc = csr_desc(g, csr_of(g), node_offsets=True)
    st = _abi.stream_ptr(torch.device(DEV))
    full = lambda k, dt=torch.int64: torch.full((k,), 77, dtype=dt, device=DEV)
    hash_, colour, edges = full(b), full(n), full(b)
    ws_bytes = lib.gnf_graph_hashes_workspace_bytes(b, n, 130)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    call = lambda cap, it, bytes_: lib.gnf_graph_hashes(C.byref(desc), cap, it, None, _abi.ptr(hash_), _abi.ptr(colour),
                                                        _abi.ptr(edges), _abi.ptr(ws), bytes_, st)
    assert call(-1, 3, ws_bytes) == -2 and call(65537, 3, ws_bytes) == -2 and call(130, 65, ws_bytes) == -2 and call(130, 3, 8) == -3
    first, found, counts = full(b, torch.int32), full(b, torch.int32), full(4)
    sizes = g.n_node.to(torch.int32)
    pair = lambda a, bytes_: lib.gnf_graph_hash_match(_abi.ptr(hash_), _abi.ptr(sizes), a, None, None, 0, _abi.ptr(first),
                                                      _abi.ptr(found), _abi.ptr(counts), _abi.ptr(ws), bytes_, st)
    assert pair(-1, 8) == -2 and pair(b, 7) == -3
    torch.cuda.synchronize()
    for x in (hash_, colour, edges, first, found, counts):
        assert (x == 77).all()
    assert call(130, 3, ws_bytes) == 0 and pair(b, 8) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hash_.cpu().numpy(), small["want"][3]["hash"])
    m = R.match(small["want"][3]["hash"], small["flat"][0], [], [])
    np.testing.assert_array_equal(first.cpu().numpy(), m["first_in_generated"])
    assert counts.tolist() == m["counts"].tolist() == [11, 9, 11, 9] and (found == -1).all()
    assert pair(0, 8) == 0                                            # a == 0: the counts are zeroed, nothing else is written
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0, 0] and first.cpu().numpy().tolist() == m["first_in_generated"].tolist()
