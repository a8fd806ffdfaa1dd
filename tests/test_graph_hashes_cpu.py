"""gnf_amd.graph_stats.graph_hashes / uniqueness_novelty, gnf_graph_hashes / gnf_graph_hash_match: everything that needs no GPU -
the reference of tests/graph_hashes_ref.py (per-edge accumulation) against a second construction (dense matrix products, one
graph at a time) and against values worked out in Python integers, the invariances the definition promises, the collisions it
admits, the isomorphism classes of the project's data sets, the match rules, the symbols, the host-side workspace sizes, the
argument validation before any launch and the no-CPU-fallback rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import graph_components_ref as CR
import graph_hashes_ref as R
import graph_stats_ref as S

NEW_SYMBOLS = ("gnf_graph_hashes_workspace_bytes", "gnf_graph_hashes", "gnf_graph_hash_match_workspace_bytes",
               "gnf_graph_hash_match")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1
KA, KB, KC, KD, SIZE = (int(v) for v in (R.KA, R.KB, R.KC, R.KD, R.SIZE))


def pmix(x):
    """mix in Python integers"""
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def u64(v):
    return int(np.asarray(v).reshape(-1)[0]) & M


# ---- the reference against a second construction ---------------------------------------------------------------------------
def _dense(n, edges, iterations, labels=None):
    """(hash, colours) of one graph as Python / numpy uint64 from its dense adjacency: the neighbour sums are A @ mix(c ^ KB)"""
    a = S.dense_adjacency(n, *edges).astype(np.uint64)
    v = a.sum(1).astype(np.uint64) if labels is None else np.asarray(labels, np.int64).view(np.uint64)
    c = R.mix(v)
    e = int(a.sum()) // 2
    h = pmix((n * SIZE + e) & M)
    h = pmix((h + sum(int(x) for x in R.mix(c ^ R.KA))) & M)
    for t in range(1, iterations + 1):
        c = R.mix(c * R.KC + a @ R.mix(c ^ R.KB) + np.uint64(t))
        h = pmix((h * KD + sum(int(x) for x in R.mix(c ^ R.KA))) & M)
    return h, c


@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 64])
def test_reference_against_dense_matrix_products(iterations):
    cases = R.small_cases() + CR.word_edge_cases()
    rng = np.random.default_rng(1)
    for how in ("one_direction", "duplicates_and_loops"):
        n_node, _, s, r = R.spell(cases, how, rng)
        labels = rng.integers(-3, 4, sum(n_node))
        for lab in (None, labels):
            got = R.hashes(n_node, s, r, iterations, lab)
            off = 0
            for g, (name, n, edges) in enumerate(cases):
                h, c = _dense(n, edges, iterations, None if lab is None else lab[off:off + n])
                assert u64(got["hash"][g]) == h, (name, how)
                np.testing.assert_array_equal(got["node_colour"][off:off + n].view(np.uint64), c, err_msg=name)
                assert got["n_edges"][g] == len(CR._simple_pairs([n], *edges)[1]) and got["n_node"][g] == n
                off += n


def test_reference_against_values_worked_out_by_hand():
    # no nodes: n = e = 0 and every sum is empty
    h0 = pmix(pmix(0))
    assert u64(R.hashes([0], [], [], 0)["hash"]) == h0
    assert u64(R.hashes([0], [], [], 1)["hash"]) == pmix(h0 * KD & M)
    assert u64(R.hashes([0], [], [], 2)["hash"]) == pmix(pmix(h0 * KD & M) * KD & M)
    # one node: degree 0
    c = pmix(0)
    one = pmix((pmix(SIZE) + pmix(c ^ KA)) & M)
    assert u64(R.hashes([1], [], [], 0)["hash"]) == one and u64(R.hashes([1], [], [], 0)["node_colour"]) == c
    c1 = pmix((c * KC + 1) & M)
    assert u64(R.hashes([1], [], [], 1)["hash"]) == pmix((one * KD + pmix(c1 ^ KA)) & M)
    # one edge: two nodes of degree 1
    c = pmix(1)
    edge0 = pmix((pmix((2 * SIZE + 1) & M) + 2 * pmix(c ^ KA)) & M)
    got = R.hashes([2], [0], [1], 0)
    assert u64(got["hash"]) == edge0 and got["node_colour"].view(np.uint64).tolist() == [c, c] and got["n_edges"].tolist() == [1]
    c1 = pmix((c * KC + pmix(c ^ KB) + 1) & M)
    got = R.hashes([2], [0], [1], 1)
    assert u64(got["hash"]) == pmix((edge0 * KD + 2 * pmix(c1 ^ KA)) & M) and got["node_colour"].view(np.uint64).tolist() == [c1, c1]
    # labels replace the degree: two nodes labelled 7 and -1 (all 64 bits set), no edge
    got = R.hashes([2], [], [], 0, labels=[7, -1])
    assert got["node_colour"].view(np.uint64).tolist() == [pmix(7), pmix(M)]
    assert u64(got["hash"]) == pmix((pmix(2 * SIZE & M) + pmix(pmix(7) ^ KA) + pmix(pmix(M) ^ KA)) & M)
    # inside a batch nothing but the rows move
    both = R.hashes([1, 0, 2], [1], [2], 1)
    assert [u64(v) for v in both["hash"]] == [u64(R.hashes([1], [], [], 1)["hash"]), pmix(h0 * KD & M), u64(R.hashes([2], [0], [1], 1)["hash"])]


@pytest.mark.parametrize("with_labels", [False, True])
def test_renumbering_the_nodes_changes_nothing(with_labels):
    rng = np.random.default_rng(8)
    for n in (5, 40, 129):
        edges = CR.sparse(n, rng, 2.5)
        labels = rng.integers(0, 3, n) if with_labels else None
        want = R.hashes([n], *edges, iterations=3, labels=labels)
        for _ in range(3):
            perm = rng.permutation(n)
            moved = None if labels is None else np.zeros(n, np.int64)
            if moved is not None:
                moved[perm] = labels
            got = R.hashes([n], *R.permuted(n, edges, perm), iterations=3, labels=moved)
            assert got["hash"][0] == want["hash"][0]
            np.testing.assert_array_equal(got["node_colour"][perm], want["node_colour"])
        if with_labels:      # and the labels do matter
            assert R.hashes([n], *edges, iterations=3)["hash"][0] != want["hash"][0]


def test_spelling_of_the_edge_list_does_not_matter():
    cases = R.small_cases()
    n_node, _, s, r = R.spell(cases, "one_direction")
    want = R.hashes(n_node, s, r, 3)
    reversed_ = R.hashes(n_node, r, s, 3)                         # every edge written the other way round
    for k in R.KEYS:
        np.testing.assert_array_equal(reversed_[k], want[k], err_msg=f"reversed {k}")
    for how in ("symmetric", "duplicates_and_loops"):
        _, _, ss, rr = R.spell(cases, how, np.random.default_rng(2))
        got = R.hashes(n_node, ss, rr, 3)
        for k in R.KEYS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{how} {k}")
    at = {c[0]: k for k, c in enumerate(cases)}
    h = want["hash"]
    assert h[at["path130"]] == h[at["path130_reversed"]] == h[at["path130_folded"]]
    assert len(set(h.tolist())) == len(cases) - 2                 # everything else is told apart
    for it in (0, 1, 2):                                          # the round salt and the round count are part of the hash
        assert not (R.hashes(n_node, s, r, it)["hash"] == want["hash"]).any()


def test_the_collisions_the_definition_admits_and_the_way_out():
    """1-dimensional colour refinement cannot separate two regular graphs of equal size and degree: PINNED, not a defect"""
    c6, tt = S.cycle(6), R.two_triangles()
    a, b = R.hashes([6], *c6, iterations=5), R.hashes([6], *tt, iterations=5)
    assert a["hash"][0] == b["hash"][0] and a["n_edges"].tolist() == b["n_edges"].tolist() == [6]
    tri_a, tri_b = R.triangles_per_node(6, c6), R.triangles_per_node(6, tt)
    assert tri_a.tolist() == [0] * 6 and tri_b.tolist() == [1] * 6
    assert R.hashes([6], *c6, iterations=5, labels=tri_a)["hash"][0] != R.hashes([6], *tt, iterations=5, labels=tri_b)["hash"][0]
    cube, wagner = R.cube(), R.wagner()
    for edges in (cube, wagner):
        assert S.node_stats(S.dense_adjacency(8, *edges))[0].tolist() == [3] * 8
    walks5 = [int(np.trace(np.linalg.matrix_power(S.dense_adjacency(8, *e).astype(np.int64), 5))) for e in (cube, wagner)]
    assert walks5[0] == 0 and walks5[1] > 0                       # bipartite against not: the two are not isomorphic
    for it in (0, 3, 8):
        assert R.hashes([8], *cube, iterations=it)["hash"][0] == R.hashes([8], *wagner, iterations=it)["hash"][0]


# ---- the project's data ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data_hashes():
    out = {}
    for name in R.DATASETS:
        nn, ne, s, r = R.dataset(name)
        out[name] = (nn, ne, s, r, {it: R.hashes(nn, s, r, it)["hash"] for it in (1, 3, 8)})
    return out


def _classes(h, nn):
    return len(set(zip(h.tolist(), nn)))


def test_isomorphism_classes_of_the_five_data_sets(data_hashes):
    want = {"caveman_small": 100, "citeseer_small": 73, "community_medium": 210, "grid": 55, "grid_small": 9}
    for name, (nn, _, _, _, by_it) in data_hashes.items():
        for it, h in by_it.items():
            assert _classes(h, nn) == want[name], (name, it)


def _nx_graphs(nx, nn, s, r):
    off = np.concatenate([[0], np.cumsum(nn)])
    gid = np.searchsorted(off, s, side="right") - 1
    graphs = []
    for g in range(len(nn)):
        x = nx.Graph()
        x.add_nodes_from(range(nn[g]))
        sel = gid == g
        x.add_edges_from((int(a), int(b)) for a, b in zip(s[sel] - off[g], r[sel] - off[g]) if a != b)
        graphs.append(x)
    return graphs


def test_same_hash_pairs_of_the_data_sets_are_isomorphic(data_hashes):
    nx = pytest.importorskip("networkx")
    pairs = 0
    for name, (nn, _, s, r, by_it) in data_hashes.items():
        graphs = _nx_graphs(nx, nn, s, r)
        h = by_it[3]
        first = {}
        for g in range(len(nn)):
            rep = first.setdefault((int(h[g]), nn[g]), g)
            if rep != g:          # isomorphism is transitive: against the class's first graph is against all of them
                assert nx.is_isomorphic(graphs[rep], graphs[g]), (name, rep, g)
                pairs += 1
        if name in ("citeseer_small", "grid_small"):      # and the classes are not too coarse: a VF2 partition of its own
            reps = []
            for x in graphs:
                if not any(nx.faster_could_be_isomorphic(x, y) and nx.is_isomorphic(x, y) for y in reps):
                    reps.append(x)
            assert len(reps) == len(first), name
    assert pairs == (200 - 73) + (100 - 55) + (12 - 9)


# ---- the match rules -------------------------------------------------------------------------------------------------------
def test_match_reference_on_a_hand_written_case():
    ha = np.array([5, 9, 5, 7, 5, 9, 3], np.int64)
    na = np.array([4, 4, 4, 0, 6, 4, 2], np.int32)        # 3: a graph without nodes; 4: hash 5 again but another size
    hb = np.array([9, 3, 9, 5], np.int64)
    nb = np.array([4, 3, 4, 6], np.int32)
    m = R.match(ha, na, hb, nb)
    assert m["first_in_generated"].tolist() == [0, 1, 0, -1, 4, 1, 6]
    assert m["match_in_training"].tolist() == [-1, 0, -1, -1, 3, 0, -1]
    assert m["counts"].tolist() == [6, 4, 3, 2]
    assert R.shares(m) == {"uniqueness": 4 / 6, "novelty": 3 / 6, "unique_novel": 2 / 6}
    none = R.match(ha, na, ha[:0], na[:0])                # b = 0: everything valid is novel
    assert none["match_in_training"].tolist() == [-1] * 7 and none["counts"].tolist() == [6, 4, 6, 4]
    same = R.match(ha, na, ha, na)                        # A = B: nothing is novel, uniqueness = classes / valid
    assert same["counts"].tolist() == [6, 4, 0, 0] and same["match_in_training"].tolist() == [0, 1, 0, -1, 4, 1, 6]
    assert R.match(ha[:0], na[:0], hb, nb)["counts"].tolist() == [0, 0, 0, 0]


def test_a_data_set_against_itself(data_hashes):
    nn, _, _, _, by_it = data_hashes["citeseer_small"]
    m = R.match(by_it[3], nn, by_it[3], nn)
    assert m["counts"].tolist() == [200, 73, 0, 0] and R.shares(m)["uniqueness"] == 73 / 200 and R.shares(m)["novelty"] == 0.0


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_graph_hashes.h (included by gnf.h), the library's exports and _abi.HASH_SYMBOLS are in step"""
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_graph_hashes.h"$', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_graph_hashes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.HASH_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS, _abi.ENCODER_TRAIN_SYMBOLS,
                  _abi.DISTANCE_SYMBOLS, _abi.INVERSE_PER_GRAPH_SYMBOLS, _abi.SPECTRA_SYMBOLS, _abi.COMPONENT_SYMBOLS):
        assert not set(_abi.HASH_SYMBOLS) & set(other)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    import importlib
    G = importlib.import_module("gnf_amd.graph_stats")        # (gnf_amd.graph_stats, the attribute, is the function)
    defines = {k: int(v) for k, v in re.findall(r"^#define GNF_(\w+) (\d+)$", text, flags=re.M)}
    assert defines == {"WL_MAX_ITERATIONS": G.WL_MAX_ITERATIONS, "WL_MAX_NODES": G.MAX_NODES_PER_GRAPH, "WL_LDS_NODES": G.WL_LDS_NODES}
    assert G.HASH_KEYS == R.KEYS and G.WL_MAX_ITERATIONS == 64 and 64 <= G.WL_LDS_NODES <= 65536
    # the constants of the definition, as the header and the kernels spell them
    src = open(os.path.join(ROOT, "graph-normalizing-flows_amd", "csrc", "gnf_graph_hashes.hip")).read()
    for k in (R.KA, R.KB, R.KC, R.KD, R.SIZE, 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB):
        assert f"0x{int(k):X}" in raw and f"0x{int(k):X}ull" in src, hex(int(k))


def test_workspace_sizes_are_host_computations_and_monotone():
    lib = _abi.lib()
    ws, stats, pair = lib.gnf_graph_hashes_workspace_bytes, lib.gnf_graph_stats_workspace_bytes, lib.gnf_graph_hash_match_workspace_bytes
    # the gnf_graph_stats workspace (bitmap, graph ids) + two colours per node + 65 table rows of one word per graph
    assert ws(4, 100, 64) == stats(4, 100, 64) + 2 * 100 * 8 + 65 * 4 * 8
    assert ws(1000, 5000, 65536) == stats(1000, 5000, 65536) + 2 * 5000 * 8 + 65 * 1000 * 8
    for a, b in ((0, 1), (1, 2), (7, 300), (63, 64), (64, 65), (4095, 4096), (4096, 4097)):
        assert ws(a, 50, 200) <= ws(b, 50, 200) and ws(3, a, 200) <= ws(3, b, 200) and ws(3, 50, a) <= ws(3, 50, b), (a, b)
    assert ws(3, 500, 200) % 8 == 0 and ws(3, 500, 200) > 0 and ws(0, 0, 0) == 0
    assert ws(-1, 10, 10) == 0 and ws(1, -1, 10) == 0 and ws(1, 10, -1) == 0 and ws(1, 10, 65537) == 0 and ws(1, 2 ** 31, 10) == 0
    assert pair(0, 0) == pair(5, 0) == pair(2 ** 31 - 1, 2 ** 31 - 1) == 8
    assert pair(-1, 0) == 0 and pair(0, -1) == 0 and pair(2 ** 31, 0) == 0 and pair(0, 2 ** 31) == 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _hash(csr=None, cap=20, it=3, labels=None, hash=P, colour=P, edges=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_hashes(C.byref(csr), cap, it, labels, hash, colour, edges, ws, ws_bytes, None)


def _match(ha=P, na=P, a=5, hb=P, nb=P, b=4, first=P, found=P, counts=P, ws=P, ws_bytes=8):
    return _abi.lib().gnf_graph_hash_match(ha, na, a, hb, nb, b, first, found, counts, ws, ws_bytes, None)


def test_graph_hashes_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _hash(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _hash(csr=_csr(b=0)) == EINVAL
    assert _abi.lib().gnf_graph_hashes(None, 20, 3, None, P, P, P, P, 1 << 20, None) == EINVAL
    for name in ("hash", "colour", "edges", "ws"):
        assert _hash(**{name: None}) == EINVAL, name
    assert _hash(csr=_csr(rowptr=None)) == EINVAL and _hash(csr=_csr(col=None)) == EINVAL
    assert _hash(cap=-1) == ESHAPE and "max_nodes_per_graph" in err()
    assert _hash(cap=65537) == ESHAPE and _hash(cap=0) == ESHAPE
    assert _hash(it=-1) == ESHAPE and "iterations" in err() and _hash(it=65) == ESHAPE
    assert _hash(csr=_csr(n=-1)) == ESHAPE and _hash(csr=_csr(e=-1)) == ESHAPE and _hash(csr=_csr(b=-1)) == ESHAPE
    assert _hash(csr=_csr(n=2 ** 31)) == ESHAPE
    need = _abi.lib().gnf_graph_hashes_workspace_bytes(3, 40, 20)
    for it in (0, 64):                                    # one size for every round count
        assert _hash(it=it, ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    for cap in (4096, 4097, 65536):                       # both routes, and the limit itself is an accepted shape
        assert _hash(cap=cap, ws_bytes=need) == EWORKSPACE
    # an empty batch is a no-op success: returns before any device work
    assert _hash(csr=_abi.GnfCsr(0, 0, 0, 0, 0, 0), cap=0, hash=None, colour=None, edges=None, ws=None, ws_bytes=0) == 0


def test_graph_hash_match_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _match(a=-1) == ESHAPE and _match(b=-1) == ESHAPE and _match(a=2 ** 31) == ESHAPE and _match(b=2 ** 31) == ESHAPE
    for name in ("ha", "na", "hb", "nb", "first", "found", "counts", "ws"):
        assert _match(**{name: None}) == EINVAL and "null" in err(), name
    assert _match(ws_bytes=7) == EWORKSPACE and "workspace" in err()
    assert _match(b=0, hb=None, nb=None, ws_bytes=7) == EWORKSPACE       # b == 0 needs no B arrays: it gets as far as the size


def test_python_layer_fails_loudly_without_a_hip_device():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd.graph_stats import evaluate_generated, graph_hashes, uniqueness_novelty
    assert gnf_amd.graph_hashes is graph_hashes and gnf_amd.uniqueness_novelty is uniqueness_novelty
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_hashes(g)
    with pytest.raises(_abi.GnfError):
        graph_hashes(g, max_nodes_per_graph=3, labels=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_abi.GnfError):
        uniqueness_novelty(g, g)
    cpu = {"hash": torch.zeros(1, dtype=torch.int64), "n_node": torch.ones(1, dtype=torch.int32)}
    with pytest.raises(_abi.GnfError):
        uniqueness_novelty(cpu, cpu)
    with pytest.raises(_abi.GnfError):
        evaluate_generated(g, g, train=g)
    with pytest.raises(ValueError):
        uniqueness_novelty({"degree_hist": None}, cpu)                      # no hashes in the dict
    with pytest.raises(ValueError):
        evaluate_generated({"degree_hist": None}, g, train=cpu)
