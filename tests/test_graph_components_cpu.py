"""gnf_amd.graph_stats.graph_components / keep_subgraphs, gnf_graph_components / gnf_graph_subgraph_*: everything that needs no
GPU - the union-find reference of tests/graph_components_ref.py against a second construction (reachability by repeated boolean
squaring of A + I) and against hand-written answers, the connectivity of the project's data sets, the symbols, the host-side
workspace sizes, the argument validation before any launch and the no-CPU-fallback rule."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import graph_components_ref as R
import graph_stats_ref as S

NEW_SYMBOLS = ("gnf_graph_components_workspace_bytes", "gnf_graph_components", "gnf_graph_subgraph_workspace_bytes",
               "gnf_graph_subgraph_count", "gnf_graph_subgraph_fill")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against a second construction ---------------------------------------------------------------------------
def _by_squaring(n, s, r):
    """the six outputs of one graph (local ids) from reach = (A + I)^(2^k), squared until it stops changing"""
    a = S.dense_adjacency(n, s, r)
    reach = a | np.eye(n, dtype=bool)
    while True:
        nxt = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if (nxt == reach).all():
            break
        reach = nxt
    comp = np.array([int(np.flatnonzero(reach[i])[0]) for i in range(n)], np.int64).reshape(n)
    size = reach.sum(1).astype(np.int64).reshape(n)
    roots = np.flatnonzero(comp == np.arange(n))
    best = max(size[roots], default=0)
    root = min((int(q) for q in roots if size[q] == best), default=-1)
    return comp, size, len(roots), int(best), root, int((a.sum(1) == 0).sum()) if n else 0


@pytest.mark.parametrize("name,n,edges", R.all_cases(), ids=[f"{k}:{c[0]}" for k, c in enumerate(R.all_cases())])
def test_reference_against_boolean_squaring(name, n, edges):
    assert n <= 130
    got = R.components([n], *edges)
    comp, size, count, best, root, isolated = _by_squaring(n, *edges)
    np.testing.assert_array_equal(got["component"], comp)
    np.testing.assert_array_equal(got["component_size"], size)
    assert [int(got[k][0]) for k in R.KEYS[2:]] == [count, best, root, isolated]
    # inside a batch the labels move by the graph's offset and nothing else changes
    both = R.components(*R.batch([("pad", 3, S.complete(3)), (name, n, edges)]))
    np.testing.assert_array_equal(both["component"][3:], comp + 3)
    assert int(both["largest_component_root"][1]) == (root + 3 if root >= 0 else -1)


def test_reference_on_the_large_cases_against_min_label_propagation():
    """the cases too large to square a matrix for (4 200 and 16 500 nodes): a third construction, vectorised - every node takes
    the smallest label among itself and its neighbours, then its label's label, until nothing changes"""
    cases = R.large_cases()
    assert [n for _, n, _ in cases] == [4200, 9, 16500]
    n_node, s, r = R.batch(cases)
    lab = np.arange(sum(n_node))
    for _ in range(len(lab)):
        new = lab.copy()
        np.minimum.at(new, s, lab[r])
        np.minimum.at(new, r, lab[s])
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    got = R.components(n_node, s, r)
    np.testing.assert_array_equal(got["component"], lab)
    np.testing.assert_array_equal(got["component_size"], np.bincount(lab, minlength=len(lab))[lab])
    assert got["n_components"].tolist() == [len(np.unique(lab[:4200])), 4, len(np.unique(lab[4209:]))]
    # what the GPU test needs of them: many components of many sizes, isolated nodes, the largest one rooted past the first word
    assert (got["n_components"][[0, 2]] > 100).all() and (got["n_isolated"][[0, 2]] > 10).all()
    assert got["largest_component_size"][0] > 64 and got["largest_component_root"][0] > 64
    assert got["largest_component_size"][2] > 64 and got["largest_component_root"][2] - 4209 > 64


def test_reference_against_hand_written_answers():
    t = R.components([9], *R.tie())
    assert t["component"].tolist() == [0, 0, 2, 3, 2, 3, 2, 3, 8] and t["component_size"].tolist() == [2, 2, 3, 3, 3, 3, 3, 3, 1]
    assert [int(t[k][0]) for k in R.KEYS[2:]] == [4, 3, 2, 1]          # the tie goes to root 2, not to the smaller {0, 1}
    s = R.components([70], *R.star_hub_last(70))
    assert s["component"].tolist() == [0] * 70 and [int(s[k][0]) for k in R.KEYS[2:]] == [1, 70, 0, 0]
    i = R.components([70], *R.no_edges(70))
    assert i["component"].tolist() == list(range(70)) and i["component_size"].tolist() == [1] * 70
    assert [int(i[k][0]) for k in R.KEYS[2:]] == [70, 1, 0, 70]
    e = R.components([0, 2, 0], [1], [0])                            # an edge between rows 0 and 1 of the middle graph
    assert [e[k].tolist() for k in R.KEYS[2:]] == [[0, 1, 0], [0, 2, 0], [-1, 0, -1], [0, 0, 0]]
    one = R.components([65], *R.single_edge(65, 63, 64))
    assert one["component"][63:].tolist() == [63, 63] and [int(one[k][0]) for k in R.KEYS[2:]] == [64, 2, 63, 63]
    for fold in (R.path(130), R.path_reversed(130), R.path_folded(130)):
        p = R.components([130], *fold)
        assert not p["component"].any() and [int(p[k][0]) for k in R.KEYS[2:]] == [1, 130, 0, 0]
    assert sorted(zip(*[v.tolist() for v in R.path_folded(7)])) == [(0, 2), (1, 0), (2, 4), (3, 1), (4, 6), (5, 3)]


def test_spelling_of_the_edge_list_does_not_matter():
    rng = np.random.default_rng(5)
    s, r = R.sparse(40, rng, 1.5)
    want = R.components([40], s, r)
    assert want["n_components"][0] > 3 and want["largest_component_size"][0] > 3      # a case with something to find
    loops = np.arange(40)
    for ss, rr in ((r, s), (np.concatenate([s, r]), np.concatenate([r, s])),
                   (np.concatenate([s, s, loops]), np.concatenate([r, r, loops]))):
        got = R.components([40], ss, rr)
        for k in R.KEYS:
            np.testing.assert_array_equal(got[k], want[k])


def test_reference_subgraph_order_loops_and_empty_graphs():
    n_node, s, r = R.batch([("tie", 9, R.tie()), ("empty", 0, R.no_edges(0)), ("K3", 3, S.complete(3))])
    keep = R.keep_mask(n_node, s, r, "largest_component")
    assert np.flatnonzero(keep).tolist() == [2, 4, 6, 9, 10, 11]
    sub = R.subgraph(n_node, s, r, keep)
    assert sub["new_id"].tolist() == [-1, -1, 0, -1, 1, -1, 2, -1, -1, 3, 4, 5] and sub["node_index"].tolist() == [2, 4, 6, 9, 10, 11]
    assert sub["new_n_node"].tolist() == [3, 0, 3] and sub["n_edge"].tolist() == [4, 0, 6]
    assert sub["receivers"].tolist() == [0, 1, 1, 2, 3, 3, 4, 4, 5, 5] and sub["senders"].tolist() == [1, 0, 2, 1, 4, 5, 3, 5, 3, 4]
    assert sub["rowptr"].tolist() == [0, 1, 3, 4, 6, 8, 10]
    loops = R.subgraph(n_node, s, r, keep, self_loops=True)
    assert loops["receivers"][:7].tolist() == [0, 0, 1, 1, 1, 2, 2] and loops["senders"][:7].tolist() == [0, 1, 0, 1, 2, 1, 2]
    assert loops["n_edge"].tolist() == [7, 0, 9]
    assert np.flatnonzero(R.keep_mask(n_node, s, r, "non_isolated")).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]
    # a mask that cuts a component: only the edges with both ends kept survive
    cut = R.subgraph(n_node, s, r, R.keep_mask(n_node, s, r, "mask", [0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1]))
    assert cut["new_n_node"].tolist() == [4, 0, 1] and cut["n_edge"].tolist() == [0, 0, 0] and len(cut["senders"]) == 0


def test_every_training_graph_is_connected_and_has_no_isolated_node():
    """what makes "fell apart" a property of GENERATED graphs only: all 622 graphs of data/*.npz are one component each"""
    total = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "data", "*.npz"))):
        d = np.load(path)
        n_node, n_edge = d["n_node"].astype(np.int64), d["n_edge"].astype(np.int64)
        off = np.repeat(np.concatenate([[0], np.cumsum(n_node)[:-1]]), n_edge)
        c = R.components(n_node, d["senders"].astype(np.int64) + off, d["receivers"].astype(np.int64) + off)
        assert (c["n_components"] == 1).all() and not c["n_isolated"].any(), path
        np.testing.assert_array_equal(c["largest_component_size"], n_node)
        total += len(n_node)
    assert total == 622


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_graph_components.h (included by gnf.h), the library's exports and _abi.COMPONENT_SYMBOLS are in step"""
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_graph_components.h"$', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_graph_components.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.COMPONENT_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS, _abi.ENCODER_TRAIN_SYMBOLS,
                  _abi.DISTANCE_SYMBOLS, _abi.INVERSE_PER_GRAPH_SYMBOLS, _abi.SPECTRA_SYMBOLS):
        assert not set(_abi.COMPONENT_SYMBOLS) & set(other)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    import importlib
    G = importlib.import_module("gnf_amd.graph_stats")        # (gnf_amd.graph_stats, the attribute, is the function)
    defines = {k: int(v) for k, v in re.findall(r"^#define GNF_(\w+) (\d+)$", text, flags=re.M)}
    assert defines == {"COMPONENTS_MAX_NODES": G.MAX_NODES_PER_GRAPH, "KEEP_LARGEST_COMPONENT": _abi.GNF_KEEP_LARGEST_COMPONENT,
                       "KEEP_NON_ISOLATED": _abi.GNF_KEEP_NON_ISOLATED, "KEEP_MASK": _abi.GNF_KEEP_MASK}
    assert G.COMPONENT_KEYS == R.KEYS and G.MAX_NODES_PER_GRAPH == 65536


def test_workspace_sizes_are_host_computations_and_monotone():
    lib = _abi.lib()
    comp, sub, stats = lib.gnf_graph_components_workspace_bytes, lib.gnf_graph_subgraph_workspace_bytes, lib.gnf_graph_stats_workspace_bytes
    # the gnf_graph_stats workspace (bitmap, graph ids) + one int32 per node, in whole 8-byte words
    assert comp(4, 100, 64) == stats(4, 100, 64) + 400 == 100 * 8 + 400 + 400
    assert comp(3, 7, 200) == stats(3, 7, 200) + 32 and comp(1000, 5000, 65536) == stats(1000, 5000, 65536) + 20000
    for ws in (comp, sub):
        for a, b in ((0, 1), (1, 2), (7, 300), (300, 301), (63, 64), (64, 65), (4095, 4096)):
            assert ws(a, 50, 200) <= ws(b, 50, 200) and ws(3, a, 200) <= ws(3, b, 200) and ws(3, 50, a) <= ws(3, 50, b), (a, b)
        assert ws(3, 500, 200) % 8 == 0 and ws(3, 500, 200) > 0
        # 0 for arguments that no call accepts
        assert ws(-1, 10, 10) == 0 and ws(1, -1, 10) == 0 and ws(1, 10, -1) == 0 and ws(1, 10, 65537) == 0
    assert sub(3, 500, 200) > comp(3, 500, 200)
    assert comp(2, 40000, 65536) > 0 and sub(2, 32767, 65536) > 0
    assert sub(2, 32768, 65536) == 0 and sub(1, 2 ** 31 - 1, 1) == 0      # n_nodes * (max_nodes_per_graph + 1) > INT32_MAX
    assert sub(1, (2 ** 31 - 1) // 2, 1) > 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _comp(csr=None, cap=20, comp=P, size=P, count=P, lsize=P, lroot=P, iso=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_components(C.byref(csr), cap, comp, size, count, lsize, lroot, iso, ws, ws_bytes, None)


def _count(csr=None, cap=20, rule=0, mask=None, loops=0, new_id=P, new_n=P, rowptr=P, n_edge=P, totals=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_subgraph_count(C.byref(csr), cap, rule, mask, loops, new_id, new_n, rowptr, n_edge, totals, ws,
                                               ws_bytes, None)


def _fill(b=3, n=40, cap=20, rowptr=P, ncap=40, ecap=100, index=P, snd=P, rcv=P, ws=P, ws_bytes=1 << 20):
    return _abi.lib().gnf_graph_subgraph_fill(b, n, cap, rowptr, ncap, ecap, index, snd, rcv, ws, ws_bytes, None)


EMPTY = lambda: _abi.GnfCsr(0, 0, 0, 0, 0, 0)


def test_graph_components_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _comp(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _comp(csr=_csr(b=0)) == EINVAL
    assert _abi.lib().gnf_graph_components(None, 20, P, P, P, P, P, P, P, 1 << 20, None) == EINVAL
    for name in ("comp", "size", "count", "lsize", "lroot", "iso", "ws"):
        assert _comp(**{name: None}) == EINVAL, name
    assert _comp(csr=_csr(rowptr=None)) == EINVAL and _comp(csr=_csr(col=None)) == EINVAL
    assert _comp(cap=-1) == ESHAPE and "max_nodes_per_graph" in err()
    assert _comp(cap=65537) == ESHAPE and _comp(cap=0) == ESHAPE
    assert _comp(csr=_csr(n=-1)) == ESHAPE and _comp(csr=_csr(e=-1)) == ESHAPE and _comp(csr=_csr(b=-1)) == ESHAPE
    assert _comp(csr=_csr(n=2 ** 31)) == ESHAPE
    need = _abi.lib().gnf_graph_components_workspace_bytes(3, 40, 20)
    assert _comp(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _comp(cap=65536, ws_bytes=need) == EWORKSPACE          # the limit itself is an accepted shape
    # an empty batch is a no-op success: returns before any device work
    assert _comp(csr=EMPTY(), cap=0, comp=None, size=None, count=None, lsize=None, lroot=None, iso=None, ws=None, ws_bytes=0) == 0


def test_graph_subgraph_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    lib = _abi.lib()
    assert _count(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert lib.gnf_graph_subgraph_count(None, 20, 0, None, 0, P, P, P, P, P, P, 1 << 20, None) == EINVAL
    for name in ("new_id", "new_n", "rowptr", "n_edge", "totals", "ws"):
        assert _count(**{name: None}) == EINVAL, name
    assert _count(rule=2, mask=None) == EINVAL and "mask" in err()
    assert _count(rule=3) == EINVAL and _count(rule=-1) == EINVAL and "rule" in err()
    assert _count(loops=2) == EINVAL and _count(loops=-1) == EINVAL
    assert _count(cap=-1) == ESHAPE and _count(cap=65537) == ESHAPE and _count(cap=0) == ESHAPE
    assert _count(csr=_csr(n=-1)) == ESHAPE and _count(csr=_csr(b=-1)) == ESHAPE
    assert _count(csr=_csr(n=32768), cap=65536) == ESHAPE and "int32" in err()
    need = lib.gnf_graph_subgraph_workspace_bytes(3, 40, 20)
    for rule, mask in ((0, None), (1, None), (2, P)):
        assert _count(rule=rule, mask=mask, ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _count(csr=_csr(n=32767), cap=65536, ws_bytes=need) == EWORKSPACE      # the limit itself is an accepted shape
    assert _count(csr=EMPTY(), cap=0, new_id=None, new_n=None, rowptr=None, n_edge=None, totals=None, ws=None, ws_bytes=0) == 0
    # fill
    assert _fill(b=-1) == ESHAPE and _fill(n=-1) == ESHAPE and _fill(cap=-1) == ESHAPE and _fill(cap=65537) == ESHAPE
    assert _fill(cap=0) == ESHAPE and _fill(ncap=-1) == ESHAPE and _fill(ecap=-1) == ESHAPE and _fill(n=32768, cap=65536) == ESHAPE
    for name in ("rowptr", "index", "snd", "rcv", "ws"):
        assert _fill(**{name: None}) == EINVAL, name
    assert _fill(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _fill(ncap=0, ecap=0, index=None, snd=None, rcv=None, ws_bytes=need - 1) == EWORKSPACE
    # nothing to do: no launch
    assert _fill(b=0, n=0, cap=0, rowptr=None, ncap=0, ecap=0, index=None, snd=None, rcv=None, ws=None, ws_bytes=0) == 0
    assert _fill(ncap=0, ecap=0, index=None, snd=None, rcv=None, ws_bytes=need) == 0


def test_python_layer_fails_loudly_without_a_hip_device():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd.graph_stats import evaluate_generated, graph_components, keep_subgraphs
    assert gnf_amd.graph_components is graph_components and gnf_amd.keep_subgraphs is keep_subgraphs
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_components(g)
    with pytest.raises(_abi.GnfError):
        graph_components(g, max_nodes_per_graph=3)
    for keep in ("largest_component", "non_isolated", torch.ones(3, dtype=torch.bool)):
        with pytest.raises(_abi.GnfError):
            keep_subgraphs(g, keep)
    with pytest.raises(_abi.GnfError):
        evaluate_generated(g, g, keep="largest_component")
    with pytest.raises(ValueError):
        evaluate_generated({"degree_hist": None}, g, keep="largest_component")      # statistics cannot be reduced
