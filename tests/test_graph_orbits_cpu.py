"""gnf_amd.graph_stats.graph_orbits / orbit_mmd, gnf_graph_orbits / gnf_vec_mmd_i64: everything that needs no GPU - the pinned
orbit rows of include/gnf_graph_orbits.h's definition on the brute-force reference the GPU tests compare against, identities that hold
for any graph, a cross-check of its classification with networkx, the vector MMD reference, the symbols, the host-side
workspace sizes, the argument validation before any launch and the no-CPU-fallback rule."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import graph_orbits_ref as R
import graph_stats_ref as S

NEW_SYMBOLS = ("gnf_graph_orbits_workspace_bytes", "gnf_graph_orbits", "gnf_vec_mmd_workspace_bytes", "gnf_vec_mmd_i64")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


def _orbits(n, edges):
    return R.node_orbits(S.dense_adjacency(n, *edges))


def _row(**kw):
    row = [0] * 15
    for k, v in kw.items():
        row[int(k[1:])] = v
    return row


# ---- pinned values ---------------------------------------------------------------------------------------------------------
def test_pinned_orbit_rows():
    assert _orbits(5, S.complete(5)).tolist() == [_row(o0=4, o3=6, o14=4)] * 5
    assert _orbits(4, S.cycle(4)).tolist() == [_row(o0=2, o1=2, o2=1, o8=1)] * 4
    assert _orbits(7, S.cycle(7)).tolist() == [_row(o0=2, o1=2, o2=1, o4=2, o5=2)] * 7
    assert _orbits(7, S.star(7)).tolist() == [_row(o0=6, o2=15, o7=20)] + [_row(o0=1, o1=5, o6=10)] * 6
    assert _orbits(10, R.petersen()).tolist() == [[3, 6, 3, 0, 12, 12, 3, 1, 0, 0, 0, 0, 0, 0, 0]] * 10
    assert _orbits(6, R.complete_bipartite(3, 3)).tolist() == [[3, 6, 3, 0, 0, 0, 3, 1, 6, 0, 0, 0, 0, 0, 0]] * 6
    assert _orbits(4, R.tailed_triangle()).tolist() == [_row(o0=3, o2=2, o3=1, o11=1), _row(o0=2, o1=1, o3=1, o10=1),
                                                        _row(o0=2, o1=1, o3=1, o10=1), _row(o0=1, o1=2, o9=1)]
    assert _orbits(4, R.chorded_cycle()).tolist() == [_row(o0=3, o2=1, o3=2, o13=1), _row(o0=2, o1=2, o3=1, o12=1)] * 2


def test_small_and_empty_graphs():
    assert _orbits(0, S.complete(0)).shape == (0, 15) and _orbits(1, S.complete(1)).tolist() == [[0] * 15]
    assert _orbits(2, S.complete(2)).tolist() == [_row(o0=1)] * 2
    assert _orbits(3, S.complete(3)).tolist() == [_row(o0=2, o3=1)] * 3
    out = R.graph_orbits([0, 3, 0, 2], [0, 1, 3], [1, 2, 4])
    assert out["orbit_sums"].tolist() == [[0] * 15, _row(o0=4, o1=2, o2=1), [0] * 15, _row(o0=2)]
    assert out["orbit_mean"][1].tolist() == [4 / 3, 2 / 3, 1 / 3] + [0.0] * 12 and not out["orbit_mean"][0].any()


def test_the_graph_model_ignores_spelling():
    s, r = S.gnp(15, 0.4, np.random.default_rng(3))
    want = _orbits(15, (s, r))
    loops = np.arange(15)
    for ss, rr in ((r, s), (np.concatenate([s, r, loops]), np.concatenate([r, s, loops])),
                   (np.concatenate([s, s]), np.concatenate([r, r]))):
        np.testing.assert_array_equal(_orbits(15, (ss, rr)), want)


# ---- identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(12, 0.6, 0), (25, 0.3, 1), (40, 0.15, 2), (40, 0.3, 3)])
def test_identities_on_random_graphs(n, p, seed):
    s, r = S.gnp(n, p, np.random.default_rng(seed))
    a = S.dense_adjacency(n, s, r)
    o = R.node_orbits(a)
    deg, tri = S.node_stats(a)
    np.testing.assert_array_equal(o[:, 0], deg)
    np.testing.assert_array_equal(o[:, 3], tri)
    m = a.astype(np.int64)
    n_tri = int(np.trace(m @ m @ m)) // 6
    n_k4 = sum(1 for i in range(n) for j in range(i + 1, n) if a[i, j] for k in range(j + 1, n) if a[i, k] and a[j, k]
               for l in range(k + 1, n) if a[i, l] and a[j, l] and a[k, l])
    tot = o.sum(0)
    assert tot[3] == 3 * n_tri and tot[14] == 4 * n_k4
    assert tot[0] == 2 * len(s) and tot[1] == 2 * tot[2]
    # inside one graphlet the column sums stand in the ratio of the orbit sizes
    assert tot[4] == tot[5]                                              # path4: 2 ends, 2 inner
    assert tot[6] == 3 * tot[7]                                          # star: 3 leaves, 1 centre
    assert tot[9] == tot[11] and tot[10] == 2 * tot[11]                  # tailed triangle: 1, 2, 1
    assert tot[12] == tot[13]                                            # chorded 4-cycle: 2, 2
    assert tot[8] % 4 == 0 and tot[14] % 4 == 0 and tot[3] % 3 == 0
    for orb, size in R.ORBIT_SIZE.items():
        assert tot[orb] % size == 0, orb


def test_classification_against_networkx():
    nx = pytest.importorskip("networkx")
    shapes = {"edge": nx.path_graph(2), "path3": nx.path_graph(3), "triangle": nx.complete_graph(3),
              "path4": nx.path_graph(4), "star4": nx.star_graph(3), "cycle4": nx.cycle_graph(4),
              "tailed_triangle": nx.Graph([(0, 1), (1, 2), (2, 0), (0, 3)]),
              "chorded_cycle": nx.Graph([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]), "complete4": nx.complete_graph(4)}
    assert len(shapes) == 9 == len(set(R.GRAPHLETS.values()))
    rng = np.random.default_rng(11)
    s, r = S.gnp(30, 0.3, rng)
    a = S.dense_adjacency(30, s, r)
    g = nx.Graph()
    g.add_nodes_from(range(30))
    g.add_edges_from(zip(s.tolist(), r.tolist()))
    subsets = R.connected_subsets(a)
    assert len(set(subsets)) == len(subsets)
    seen = set()
    for idx in rng.choice(len(subsets), size=400, replace=False):
        nodes = subsets[int(idx)]
        sub = g.subgraph(nodes)
        assert nx.is_connected(sub)
        name, deg = R.classify(a.tolist(), nodes)
        assert [sub.degree(u) for u in nodes] == deg
        for other, shape in shapes.items():
            assert nx.is_isomorphic(sub, shape) == (other == name), (nodes, name, other)
        seen.add(name)
    assert len(seen) >= 7
    # and nothing is missed: every connected 4-subset, by plain enumeration of all of them on a smaller graph
    small = a[:14, :14]
    import itertools
    want = {c for k in (2, 3, 4) for c in itertools.combinations(range(14), k)
            if nx.is_connected(nx.Graph(small[np.ix_(c, c)].astype(int)))}
    assert set(R.connected_subsets(small)) == want


# ---- vector MMD reference --------------------------------------------------------------------------------------------------
def test_vector_mmd_reference():
    rng = np.random.default_rng(0)
    sums, cnt = rng.integers(0, 500, size=(5, 15)), rng.integers(1, 9, size=5)
    assert R.vec_mmd2(sums, cnt, sums, cnt) == 0.0
    assert R.vec_mmd_sums(sums, cnt, sums, cnt)[3:].tolist() == [5.0, 5.0]
    x, y = np.array([[30, 0, 12]]), np.array([[0, 40, 12]])
    d2 = (30 / 2 - 0.0) ** 2 + (0.0 - 40 / 4) ** 2 + (12 / 2 - 12 / 4) ** 2
    for sigma in (30.0, 5.0):
        assert R.vec_mmd2(x, [2], y, [4], sigma) == pytest.approx(2.0 - 2.0 * math.exp(-d2 / (2.0 * sigma * sigma)), abs=1e-15)
    # graphs without nodes are left out and counted out
    with_empty = R.vec_mmd_sums(np.vstack([sums, np.zeros((1, 15), int)]), list(cnt) + [0], sums[:3], cnt[:3])
    np.testing.assert_array_equal(with_empty, R.vec_mmd_sums(sums, cnt, sums[:3], cnt[:3]))
    assert with_empty[3:].tolist() == [5.0, 3.0]
    with pytest.raises(ValueError):
        R.vec_mmd2(np.zeros((2, 15), int), [0, 0], sums, cnt)


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_graph_orbits.h (included by gnf.h), the library's exports and _abi.ORBIT_SYMBOLS are in step"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_graph_orbits.h"$', main, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_graph_orbits.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.ORBIT_SYMBOLS)
    assert not set(_abi.ORBIT_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION


def test_workspace_sizes_are_host_computations_and_monotone():
    lib = _abi.lib()
    ws = lib.gnf_graph_orbits_workspace_bytes
    # bitmap [N][ceil(max / 64)] uint64 | graph id, degree and triangles of every node [N] int32 each
    assert ws(4, 100, 64) == 100 * 1 * 8 + 3 * 100 * 4
    assert ws(4, 100, 65) == 100 * 2 * 8 + 3 * 100 * 4
    assert ws(4, 101, 64) > ws(4, 100, 64) and ws(4, 100, 63) <= ws(4, 100, 64) and ws(4, 101, 64) % 8 == 0
    for a, b in ((1, 2), (7, 300), (300, 301), (0, 8192)):
        assert ws(a, 50, 40) <= ws(b, 50, 40) and ws(3, a, 40) <= ws(3, b, 40) and ws(3, 50, a) <= ws(3, 50, b)
    assert ws(-1, 10, 10) == 0 and ws(0, 0, 0) == 0
    mm = lib.gnf_vec_mmd_workspace_bytes
    assert mm(7, 5) == 12 * 2 * 8 and mm(0, 0) == 0 and mm(-1, 3) == 0
    for a, b in ((1, 2), (7, 300)):
        assert mm(a, 5) < mm(b, 5) and mm(5, a) < mm(5, b)


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _orb(csr=None, cap=20, orbits=P, ld=15, sums=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_orbits(C.byref(csr), cap, orbits, ld, sums, ws, ws_bytes, None)


def _mmd(xa=P, ca=P, a=7, lda=15, xb=P, cb=P, b=5, ldb=16, width=15, sigma=30.0, out=P, ws=P, ws_bytes=1 << 20):
    return _abi.lib().gnf_vec_mmd_i64(xa, ca, a, lda, xb, cb, b, ldb, width, sigma, out, ws, ws_bytes, None)


def test_graph_orbits_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _orb(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _orb(csr=_csr(b=0)) == EINVAL
    assert _abi.lib().gnf_graph_orbits(None, 20, P, 15, P, P, 1 << 20, None) == EINVAL
    for name in ("orbits", "sums", "ws"):
        assert _orb(**{name: None}) == EINVAL, name
    assert _orb(csr=_csr(rowptr=None)) == EINVAL and _orb(csr=_csr(col=None)) == EINVAL
    assert _orb(ld=14) == ESHAPE and "ld_orbits" in err() and _orb(ld=0) == ESHAPE
    assert _orb(cap=-1) == ESHAPE and _orb(cap=8193) == ESHAPE and _orb(cap=0) == ESHAPE
    assert _orb(csr=_csr(n=-1)) == ESHAPE and _orb(csr=_csr(e=-1)) == ESHAPE
    need = _abi.lib().gnf_graph_orbits_workspace_bytes(3, 40, 20)
    assert _orb(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _orb(cap=8192, ws_bytes=need) == EWORKSPACE             # the bound itself is accepted, its bitmap is larger
    # an empty batch is a no-op success: returns before any device work
    assert _orb(csr=_abi.GnfCsr(0, 0, 0, 0, 0, 0), cap=0, orbits=None, sums=None, ws=None, ws_bytes=0) == 0


def test_vec_mmd_validation_without_a_gpu():
    assert _mmd(width=16) == ESHAPE and _mmd(lda=14) == ESHAPE and _mmd(ldb=14) == ESHAPE
    assert _mmd(a=-1) == ESHAPE and _mmd(b=-1) == ESHAPE and _mmd(width=-1) == ESHAPE
    assert _mmd(sigma=0.0) == EINVAL and _mmd(sigma=-1.0) == EINVAL and _mmd(sigma=float("nan")) == EINVAL
    for name in ("xa", "ca", "xb", "cb", "out", "ws"):
        assert _mmd(**{name: None}) == EINVAL, name
    need = _abi.lib().gnf_vec_mmd_workspace_bytes(7, 5)
    assert _mmd(ws_bytes=need - 1) == EWORKSPACE
    assert "workspace" in _abi.lib().gnf_last_error().decode()


def test_python_layer_fails_loudly_without_a_hip_device():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd.graph_stats import evaluate_generated, graph_orbits, orbit_mmd
    assert gnf_amd.graph_orbits is graph_orbits and gnf_amd.orbit_mmd is orbit_mmd
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_orbits(g)
    with pytest.raises(_abi.GnfError):
        graph_orbits(g, max_nodes_per_graph=3)
    sums, cnt = torch.ones(2, 15, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_abi.GnfError):
        orbit_mmd((sums, cnt), (sums, cnt))
    with pytest.raises(_abi.GnfError):
        orbit_mmd({"orbit_sums": sums, "n_node": cnt}, (sums, cnt))
    with pytest.raises(_abi.GnfError):
        evaluate_generated(g, g, True)
