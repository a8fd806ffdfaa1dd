"""gnf_amd.graph_stats / gnf_graph_stats / gnf_hist_mmd_f64: everything that needs no GPU - closed forms and estimator pins
on the numpy reference the GPU tests compare against, optional cross-checks of that reference with networkx / scipy, the
symbols, the host-side workspace sizes, the argument validation before any launch and the no-CPU-fallback rule."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import graph_stats_ref as R

NEW_SYMBOLS = ("gnf_graph_stats_workspace_bytes", "gnf_graph_stats", "gnf_hist_mmd_workspace_bytes", "gnf_hist_mmd_f64")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


def _one(n, edges, bins=100):
    s, r = edges
    return R.graph_stats([n], s, r, bins=bins)


# ---- closed forms on the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 7, 65])
def test_complete_graph(n):
    st = _one(n, R.complete(n))
    assert (st["degree"] == n - 1).all() and (st["triangles"] == math.comb(n - 1, 2)).all()
    assert st["clustering_hist"][0, 99] == n and st["clustering_hist"].sum() == n
    assert st["degree_hist"][0, n - 1] == n and st["degree_hist"].shape == (1, n)
    assert st["n_edges"][0] == math.comb(n, 2) and st["n_triangles"][0] == math.comb(n, 3)
    assert (st["clustering"] == 1.0).all()


@pytest.mark.parametrize("n", [4, 5, 63])
def test_cycle_and_star_have_no_triangles(n):
    for edges, n_edges in ((R.cycle(n), n), (R.star(n), n - 1)):
        st = _one(n, edges)
        assert (st["triangles"] == 0).all() and (st["clustering"] == 0.0).all()
        assert st["clustering_hist"][0, 0] == n and st["n_edges"][0] == n_edges and st["n_triangles"][0] == 0
    assert (_one(n, R.cycle(n))["degree"] == 2).all()
    assert _one(n, R.star(n))["degree"].tolist() == [n - 1] + [1] * (n - 1)


def test_triangle_with_a_pendant():
    st = _one(4, ([0, 1, 2, 2], [1, 2, 0, 3]))
    assert st["degree"].tolist() == [2, 2, 3, 1] and st["triangles"].tolist() == [1, 1, 1, 0]
    assert st["clustering"][2] == pytest.approx(1.0 / 3.0)
    assert R.clustering_bin(3, 1, 100) == 33
    assert st["clustering_hist"][0, 99] == 2 and st["clustering_hist"][0, 33] == 1 and st["clustering_hist"][0, 0] == 1


def test_bin_edge_is_exact():
    """d = 5, T = 1: c = 0.1 sits exactly on an edge - bin 10 (the exact rational; float rounding of the edge is irrelevant)"""
    assert R.clustering_bin(5, 1, 100) == 10
    s = [0, 0, 0, 0, 0, 1]
    r = [1, 2, 3, 4, 5, 2]
    st = _one(6, (s, r))
    assert st["degree"][0] == 5 and st["triangles"][0] == 1 and st["clustering_hist"][0, 10] == 1
    assert R.clustering_bin(0, 0, 100) == 0 and R.clustering_bin(1, 0, 100) == 0 and R.clustering_bin(2, 1, 100) == 99
    assert R.clustering_bin(2, 1, 1) == 0


def test_the_graph_model_ignores_spelling():
    rng = np.random.default_rng(3)
    s, r = R.gnp(20, 0.3, rng)
    want = _one(20, (s, r))
    loops = np.arange(20)
    for ss, rr in ((r, s), (np.concatenate([s, r, loops]), np.concatenate([r, s, loops])),
                   (np.concatenate([s, s]), np.concatenate([r, r]))):
        got = _one(20, (ss, rr))
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---- estimator pins --------------------------------------------------------------------------------------------------------
def test_mmd_of_two_point_masses():
    a, b = np.array([[1, 0]]), np.array([[0, 3]])
    assert R.mmd2(a, b) == pytest.approx(2.0 - 2.0 * math.exp(-0.5), abs=1e-15)
    assert R.mmd_sums(a, b).tolist() == pytest.approx([1.0, 1.0, math.exp(-0.5), 1.0, 1.0])


def test_identical_sets_give_zero():
    h = np.random.default_rng(0).integers(0, 9, size=(5, 12))
    assert abs(R.mmd2(h, h)) <= 1e-15 and abs(R.mmd2(h, h, "gaussian_tv", 0.3)) <= 1e-15
    assert abs(R.mmd2(h, 7 * h)) <= 1e-15          # counts are normalised


def test_distances():
    for i, j, scale in ((0, 5, 1.0), (7, 2, 100.0), (3, 3, 2.0)):
        x, y = np.zeros(9), np.zeros(9)
        x[i], y[j] = 1.0, 1.0
        assert R.emd(x, y, scale) == abs(i - j) / scale
        assert R.tv(x, y) == (0.0 if i == j else 1.0)
    assert R.emd([1.0], [1.0]) == 0.0                   # one bin: no boundary to carry mass over
    assert R.tv([0.5, 0.5, 0, 0], [0, 0, 0.25, 0.75]) == 1.0


def test_padding_and_empty_rows():
    a = np.array([[2, 2, 0], [0, 0, 0]])
    b = np.array([[0, 0, 0, 0, 4], [0, 0, 0, 0, 0], [1, 1, 0, 0, 0]])
    s = R.mmd_sums(a, b)
    assert s[3] == 1 and s[4] == 2
    w = R.emd([0.5, 0.5, 0, 0, 0], [0, 0, 0, 0, 1])
    assert w == 3.5
    assert s[2] == pytest.approx(math.exp(-0.5 * 3.5 ** 2) + 1.0)
    with pytest.raises(ValueError):
        R.mmd2(np.zeros((2, 3), int), b)


# ---- optional cross-checks of the reference --------------------------------------------------------------------------------
def test_reference_against_networkx():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(40)
    s, r = R.gnp(40, 0.3, rng)
    st = _one(40, (s, r))
    g = nx.Graph()
    g.add_nodes_from(range(40))
    g.add_edges_from(zip(s.tolist(), r.tolist()))
    tri, clu = nx.triangles(g), nx.clustering(g)
    assert st["triangles"].tolist() == [tri[i] for i in range(40)]
    assert st["degree"].tolist() == [g.degree(i) for i in range(40)]
    np.testing.assert_allclose(st["clustering"], [clu[i] for i in range(40)], rtol=1e-14, atol=0)
    hist = nx.degree_histogram(g)
    assert st["degree_hist"][0, :len(hist)].tolist() == hist and st["degree_hist"][0, len(hist):].sum() == 0
    assert st["n_edges"][0] == g.number_of_edges() and st["n_triangles"][0] == sum(tri.values()) // 3


def test_reference_emd_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(41)
    for _ in range(5):
        x, y = rng.random(30), rng.random(30)
        x, y = x / x.sum(), y / y.sum()
        want = stats.wasserstein_distance(np.arange(30), np.arange(30), x, y)
        assert R.emd(x, y) == pytest.approx(want, rel=1e-12, abs=1e-14)


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        assert s in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert lib.gnf_abi_version() == 10 and len(_abi.EXPORTED_SYMBOLS) == 41


def test_workspace_sizes_are_host_computations_and_monotone():
    lib = _abi.lib()
    ws = lib.gnf_graph_stats_workspace_bytes
    # bitmap [N][ceil(max / 64)] uint64 | graph id of every node [N] int32
    assert ws(4, 100, 64) == 100 * 1 * 8 + 100 * 4
    assert ws(4, 100, 65) == 100 * 2 * 8 + 100 * 4
    assert ws(4, 101, 64) > ws(4, 100, 64) and ws(4, 100, 63) <= ws(4, 100, 64)
    for a, b in ((1, 2), (7, 300), (300, 301), (0, 65536)):
        assert ws(a, 50, 40) <= ws(b, 50, 40) and ws(3, a, 40) <= ws(3, b, 40) and ws(3, 50, a) <= ws(3, 50, b)
    assert ws(-1, 10, 10) == 0 and ws(0, 0, 0) == 0
    mm = lib.gnf_hist_mmd_workspace_bytes
    assert mm(7, 5) == 12 * 4 * 8 and mm(0, 0) == 0 and mm(-1, 3) == 0
    for a, b in ((1, 2), (7, 300)):
        assert mm(a, 5) < mm(b, 5) and mm(5, a) < mm(5, b)


def _csr(n=40, e=100, b=3, off=P):
    return _abi.GnfCsr(P, P, n, e, off, b)


def _stats(csr=None, cap=20, bins=100, deg=P, tri=P, dh=P, ch=P, ne=P, nt=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_stats(C.byref(csr), cap, bins, deg, tri, dh, ch, ne, nt, ws, ws_bytes, None)


def _mmd(ha=P, a=7, lda=10, la=10, hb=P, b=5, ldb=12, lb=12, kernel=0, sigma=1.0, scale=1.0, out=P, ws=P, ws_bytes=1 << 20):
    return _abi.lib().gnf_hist_mmd_f64(ha, a, lda, la, hb, b, ldb, lb, kernel, sigma, scale, out, ws, ws_bytes, None)


def test_graph_stats_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _stats(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _stats(csr=_csr(b=0)) == EINVAL
    assert _abi.lib().gnf_graph_stats(None, 20, 100, P, P, P, P, P, P, P, 1 << 20, None) == EINVAL
    for name in ("deg", "tri", "dh", "ch", "ne", "nt", "ws"):
        assert _stats(**{name: None}) == EINVAL, name
    assert _stats(bins=0) == ESHAPE and _stats(bins=-3) == ESHAPE
    assert _stats(cap=-1) == ESHAPE and _stats(cap=65537) == ESHAPE and "int32" in err()
    assert _stats(cap=0) == ESHAPE
    need = _abi.lib().gnf_graph_stats_workspace_bytes(3, 40, 20)
    assert _stats(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _stats(cap=65536, ws_bytes=need) == EWORKSPACE          # the bound itself is accepted, its bitmap is larger
    # an empty batch is a no-op success: returns before any device work
    assert _stats(csr=_abi.GnfCsr(0, 0, 0, 0, 0, 0), cap=0, deg=None, tri=None, dh=None, ch=None, ne=None, nt=None, ws=None,
                  ws_bytes=0) == 0


# ---- one single-fault table for the six batch entry points on the adjacency bitmap -----------------------------------------
OUT = object()   # an output pointer: non-null in a fault row, null in the empty batch
_BATCH = {       # entry point: (largest max_nodes_per_graph, the arguments between max_nodes_per_graph and the workspace)
    "gnf_graph_stats": (65536, (100, OUT, OUT, OUT, OUT, OUT, OUT)),
    "gnf_graph_orbits": (8192, (OUT, 15, OUT)),
    "gnf_graph_spectra": (2048, (OUT, OUT, 200, -1e-5, 2.0)),
    "gnf_graph_components": (65536, (OUT,) * 6),
    "gnf_graph_subgraph_count": (65536, (_abi.GNF_KEEP_LARGEST_COMPONENT, None, 0, OUT, OUT, OUT, OUT, OUT)),
    "gnf_graph_hashes": (65536, (3, None, OUT, OUT, OUT)),
}
_FAULTS = {      # row: (GnfCsr fields that differ from the valid batch, None = a null csr; max_nodes_per_graph; the code)
    "null_csr": (None, 20, EINVAL),
    "node_offsets_null_with_graphs": (dict(off=None), 20, EINVAL),
    "node_offsets_null_without_graphs": (dict(off=None, b=0), 20, EINVAL),
    "node_offsets_null_with_graphs_without_nodes": (dict(off=None, n=0, e=0), 20, EINVAL),
    "no_graphs_with_nodes": (dict(b=0), 20, EINVAL),
    "rowptr_null": (dict(rowptr=None), 20, EINVAL),
    "col_null_with_edges": (dict(col=None), 20, EINVAL),
    "negative_n_nodes": (dict(n=-1), 20, ESHAPE),
    "negative_n_edges": (dict(e=-1), 20, ESHAPE),
    "negative_n_graphs": (dict(b=-1), 20, ESHAPE),
    "n_graphs_2_31": (dict(b=2 ** 31), 20, ESHAPE),
    "cap_negative": ({}, -1, ESHAPE),
    "cap_above_the_limit": ({}, "limit + 1", ESHAPE),
    "cap_zero_with_nodes": ({}, 0, ESHAPE),
    # components, hashes and the extraction hold node ids in int32; stats, orbits and spectra get past the CSR checks and as
    # far as the workspace size (ws_bytes = 0: the call returns before any device work)
    "n_nodes_2_31": (dict(n=2 ** 31), 20, {"gnf_graph_stats": EWORKSPACE, "gnf_graph_orbits": EWORKSPACE,
                                          "gnf_graph_spectra": EWORKSPACE, "gnf_graph_components": ESHAPE,
                                          "gnf_graph_subgraph_count": ESHAPE, "gnf_graph_hashes": ESHAPE}),
    "empty_batch_with_null_outputs": (dict(n=0, e=0, b=0, off=None, rowptr=None, col=None), 0, 0),
}


@pytest.mark.parametrize("fault", list(_FAULTS))
@pytest.mark.parametrize("entry", list(_BATCH))
def test_batch_entry_points_share_one_fault_table(entry, fault):
    """A call with exactly one fault returns the same code from gnf_graph_stats, _orbits, _spectra, _components,
    _subgraph_count and _hashes - before any device work, so without a GPU."""
    limit, middle = _BATCH[entry]
    fields, cap, code = _FAULTS[fault]
    code = code[entry] if isinstance(code, dict) else code
    cap = limit + 1 if cap == "limit + 1" else cap
    empty = fault == "empty_batch_with_null_outputs"
    csr = None
    if fields is not None:
        f = dict(dict(rowptr=P, col=P, n=40, e=100, off=P, b=3), **fields)
        csr = C.byref(_abi.GnfCsr(f["rowptr"], f["col"], f["n"], f["e"], f["off"], f["b"]))
    out = None if empty else P
    ws_bytes = 0 if empty or fault == "n_nodes_2_31" else 1 << 20
    fn = getattr(_abi.lib(), entry)
    assert fn(csr, cap, *(out if a is OUT else a for a in middle), out, ws_bytes, None) == code


def test_hist_mmd_validation_without_a_gpu():
    assert _mmd(la=11) == ESHAPE and _mmd(lb=13) == ESHAPE
    assert _mmd(a=-1) == ESHAPE and _mmd(b=-1) == ESHAPE and _mmd(la=-1) == ESHAPE
    assert _mmd(sigma=0.0) == EINVAL and _mmd(sigma=-1.0) == EINVAL and _mmd(sigma=float("nan")) == EINVAL
    assert _mmd(scale=0.0) == EINVAL and _mmd(scale=-2.0) == EINVAL
    assert _mmd(kernel=2) == EINVAL and _mmd(kernel=-1) == EINVAL
    for name in ("ha", "hb", "out", "ws"):
        assert _mmd(**{name: None}) == EINVAL, name
    need = _abi.lib().gnf_hist_mmd_workspace_bytes(7, 5)
    assert _mmd(ws_bytes=need - 1) == EWORKSPACE
    assert "workspace" in _abi.lib().gnf_last_error().decode()


def test_python_layer_fails_loudly_without_a_hip_device():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd.graph_stats import evaluate_generated, graph_stats, hist_mmd
    assert gnf_amd.graph_stats is graph_stats and gnf_amd.hist_mmd is hist_mmd
    assert gnf_amd.evaluate_generated is evaluate_generated
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_stats(g)
    with pytest.raises(_abi.GnfError):
        graph_stats(g, max_nodes_per_graph=3)
    with pytest.raises(_abi.GnfError):
        hist_mmd(torch.ones(2, 3, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32))
    with pytest.raises(_abi.GnfError):
        evaluate_generated(g, g)
    with pytest.raises(ValueError):
        hist_mmd(torch.ones(2, 3, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32), kernel="linear")
