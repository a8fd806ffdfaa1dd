"""gnf_amd.graph_stats.graph_spectra / spectral_mmd, gnf_graph_spectra: everything that needs no GPU - closed forms that pin the
reference of tests/graph_spectra_ref.py to include/gnf_graph_spectra.h's definition, the clamped histogram, the margin condition
the GPU tests' exact histogram comparison rests on, the symbols, the host-side workspace size, the argument validation before
any launch and the no-CPU-fallback rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import graph_spectra_ref as R
import graph_stats_ref as S

NEW_SYMBOLS = ("gnf_graph_spectra_workspace_bytes", "gnf_graph_spectra")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 7, 20])
def test_complete_graph(n):
    e = R.eigenvalues(n, *S.complete(n))
    np.testing.assert_allclose(e, [0.0] + [n / (n - 1)] * (n - 1), rtol=0, atol=1e-14)


@pytest.mark.parametrize("n", [3, 4, 9, 64])
def test_cycle(n):
    want = np.sort(1.0 - np.cos(2.0 * np.pi * np.arange(n) / n))
    np.testing.assert_allclose(R.eigenvalues(n, *S.cycle(n)), want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("n", [3, 9, 30])
def test_star(n):
    np.testing.assert_allclose(R.eigenvalues(n, *S.star(n)), [0.0] + [1.0] * (n - 2) + [2.0], rtol=0, atol=1e-14)


def test_components_isolated_nodes_and_small_graphs():
    e = R.eigenvalues(10, *R.two_components_and_isolated())
    # triangle: 0, 3/2, 3/2; path on 4 nodes: 0, 1/2, 3/2, 2; three isolated nodes: three zeros
    np.testing.assert_allclose(e, [0, 0, 0, 0, 0, 0.5, 1.5, 1.5, 1.5, 2.0], rtol=0, atol=1e-14)
    assert R.eigenvalues(0, [], []).shape == (0,) and R.eigenvalues(1, [], []).tolist() == [0.0]
    np.testing.assert_allclose(R.eigenvalues(5, [], []), np.zeros(5), rtol=0, atol=0)
    np.testing.assert_allclose(R.eigenvalues(2, [0], [1]), [0.0, 2.0], rtol=0, atol=1e-15)
    lap = R.laplacian(S.dense_adjacency(4, [0, 0], [1, 2]))       # a path 1 - 0 - 2 and the isolated node 3
    h = -1.0 / np.sqrt(2.0)
    np.testing.assert_array_equal(lap, [[1, h, h, 0], [h, 1, 0, 0], [h, 0, 1, 0], [0, 0, 0, 0]])


def test_spelling_of_the_edge_list_does_not_matter():
    rng = np.random.default_rng(5)
    s, r = S.gnp(15, 0.3, rng)
    want = R.eigenvalues(15, s, r)
    loops = np.arange(15)
    for ss, rr in ((r, s), (np.concatenate([s, r]), np.concatenate([r, s])),
                   (np.concatenate([s, s, loops]), np.concatenate([r, r, loops]))):
        np.testing.assert_array_equal(R.eigenvalues(15, ss, rr), want)


def test_histogram_clamps_and_keeps_every_eigenvalue():
    assert R.bin_of([-1.0, -1e-5, 0.0, 1.0, 1.9999, 2.0, 2.0000000000000004, 7.0]).tolist() == [0, 0, 0, 100, 199, 199, 199, 199]
    assert R.bin_of([0.0, 0.49, 0.5, 2.5], 0.0, 1.0, 2).tolist() == [0, 0, 1, 1] and R.bin_of([-3.0, 3.0], 0.0, 1.0, 1).tolist() == [0, 0]
    e = R.eigenvalues(36, *R.grid(6, 6))
    assert e[-1] >= 2.0 - 1e-14                               # bipartite: the top eigenvalue is 2 up to rounding, on either side
    h = R.histogram(e)
    assert h.sum() == 36 and h[199] >= 1 and h.dtype == np.int32 and h.shape == (200,)
    out = R.graph_spectra(*R.batch(R.mixed_cases()))
    assert out["spectral_hist"].sum(1).tolist() == out["n_node"].tolist() and not out["spectral_hist"][0].any()
    assert R.edge_margin([0.25, 0.75], 0.0, 1.0, 2) == 0.25 and R.edge_margin([0.3], 0.0, 1.0, 1) == np.inf
    assert R.edge_margin([0.5 + 1e-12], 0.0, 1.0, 2) == pytest.approx(1e-12, rel=1e-3)


def _gpu_cases():
    from gnf_amd.graph_stats import SPECTRA_LDS_NODES
    return R.mixed_cases() + R.other_cases() + R.route_cases(SPECTRA_LDS_NODES)


def test_every_gpu_case_keeps_its_eigenvalues_off_the_bin_edges():
    """The condition under which an eigenvalue error of EIG_ATOL cannot move a histogram count: every case of the GPU tests
    (none left out) keeps MARGIN >> EIG_ATOL from every interior edge of the default bins.  A seeded random case that
    violates it gets another seed in graph_spectra_ref.py."""
    assert R.MARGIN >= 100 * R.EIG_ATOL
    for name, n, (s, r) in _gpu_cases():
        m = R.edge_margin(R.eigenvalues(n, s, r))
        assert m >= R.MARGIN, (name, m)


def test_case_list_is_what_the_gpu_tests_need():
    names = [c[0] for c in R.mixed_cases()]
    assert names == ["empty", "single", "edge", "triangle", "K4", "star9", "ring5", "ring17", "ring64", "ring65", "grid6x6",
                     "components", "gnp40"]
    for name, n, (s, r) in _gpu_cases():
        a = S.dense_adjacency(n, s, r)
        assert len(s) == len(r) and (n == 0 or (np.asarray(s) < n).all()), name
        if name.startswith("ring") and n >= 5:
            assert a.sum(1).min() >= 2 and a.sum(1).max() >= 3, name      # connected through the cycle, chords present
    sizes = [n for _, n, _ in R.route_cases(139)]
    assert sizes == [139, 140, 199]


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_graph_spectra.h (included by gnf.h), the library's exports and _abi.SPECTRA_SYMBOLS are in step"""
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_graph_spectra.h"$', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_graph_spectra.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.SPECTRA_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS,
                  _abi.ENCODER_TRAIN_SYMBOLS, _abi.DISTANCE_SYMBOLS, _abi.INVERSE_PER_GRAPH_SYMBOLS):
        assert not set(_abi.SPECTRA_SYMBOLS) & set(other)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    # the limits the header states are the ones the Python layer exports
    import importlib
    G = importlib.import_module("gnf_amd.graph_stats")        # (gnf_amd.graph_stats, the attribute, is the function)
    limits = {k: int(v) for k, v in re.findall(r"^#define GNF_SPECTRA_(\w+) (\d+)$", text, flags=re.M)}
    assert limits == {"MAX_NODES": G.SPECTRA_MAX_NODES_PER_GRAPH, "LDS_NODES": G.SPECTRA_LDS_NODES, "SLOTS": G.SPECTRA_SLOTS}
    assert G.SPECTRA_MAX_NODES_PER_GRAPH == 2048
    # n_lds is the largest n with 8 n^2 + 32 n + 4224 bytes inside 160 KiB, as the header derives it
    lds = lambda n: 8 * n * n + 32 * n + 4224
    assert lds(G.SPECTRA_LDS_NODES) <= 160 * 1024 < lds(G.SPECTRA_LDS_NODES + 1)


def test_workspace_size_is_a_host_computation_and_monotone():
    from gnf_amd.graph_stats import SPECTRA_LDS_NODES as NL, SPECTRA_MAX_NODES_PER_GRAPH as NMAX, SPECTRA_SLOTS as SL
    lib = _abi.lib()
    ws, stats = lib.gnf_graph_spectra_workspace_bytes, lib.gnf_graph_stats_workspace_bytes
    # LDS route: the gnf_graph_stats bitmap and nothing else
    assert ws(4, 100, 64) == stats(4, 100, 64) == 100 * 1 * 8 + 100 * 4
    assert ws(1000, 5000, NL) == stats(1000, 5000, NL)
    # workspace route: + min(n_graphs, S) slots of cap^2 doubles
    assert ws(4, 700, NL + 1) == stats(4, 700, NL + 1) + 4 * (NL + 1) ** 2 * 8
    assert ws(SL, 90000, 361) == stats(SL, 90000, 361) + SL * 361 * 361 * 8
    for b in (SL + 1, 3 * SL, 100000):                         # the slot formula once n_graphs exceeds S
        assert ws(b, 90000, 361) == stats(b, 90000, 361) + SL * 361 * 361 * 8
    assert ws(2, 4096, NMAX) == stats(2, 4096, NMAX) + 2 * NMAX * NMAX * 8
    for a, b in ((1, 2), (7, 300), (300, 301), (0, NMAX), (NL, NL + 1), (SL - 1, SL), (SL, SL + 1)):
        assert ws(a, 50, 200) <= ws(b, 50, 200) and ws(3, a, 200) <= ws(3, b, 200) and ws(3, 50, a) <= ws(3, 50, b), (a, b)
    assert ws(3, 500, 200) % 8 == 0
    # 0 for arguments that no call accepts
    assert ws(-1, 10, 10) == 0 and ws(1, -1, 10) == 0 and ws(1, 10, -1) == 0 and ws(1, 10, NMAX + 1) == 0 and ws(0, 0, 0) == 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _spec(csr=None, cap=20, eig=P, hist=P, bins=200, lo=-1e-5, hi=2.0, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_graph_spectra(C.byref(csr), cap, eig, hist, bins, lo, hi, ws, ws_bytes, None)


def test_graph_spectra_validation_without_a_gpu():
    err = lambda: _abi.lib().gnf_last_error().decode()
    assert _spec(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _spec(csr=_csr(b=0)) == EINVAL
    assert _abi.lib().gnf_graph_spectra(None, 20, P, P, 200, -1e-5, 2.0, P, 1 << 20, None) == EINVAL
    for name in ("eig", "ws"):
        assert _spec(**{name: None}) == EINVAL, name
    assert _spec(hist=None) == EINVAL and "hist" in err()
    assert _spec(csr=_csr(rowptr=None)) == EINVAL and _spec(csr=_csr(col=None)) == EINVAL
    assert _spec(cap=-1) == ESHAPE and "max_nodes_per_graph" in err()
    assert _spec(cap=2049) == ESHAPE and _spec(cap=0) == ESHAPE
    assert _spec(bins=-1) == ESHAPE and "bins" in err()
    assert _spec(lo=2.0, hi=2.0) == ESHAPE and _spec(lo=2.0, hi=1.0) == ESHAPE and _spec(hi=float("nan")) == ESHAPE
    assert _spec(csr=_csr(n=-1)) == ESHAPE and _spec(csr=_csr(e=-1)) == ESHAPE and _spec(csr=_csr(b=-1)) == ESHAPE
    need = _abi.lib().gnf_graph_spectra_workspace_bytes(3, 40, 20)
    assert _spec(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    # either side of the LDS limit and the bound itself are accepted shapes: only their workspace is larger
    assert _spec(cap=139, ws_bytes=need) == EWORKSPACE and _spec(cap=140, ws_bytes=need) == EWORKSPACE
    assert _spec(cap=2048, ws_bytes=need) == EWORKSPACE
    # without a histogram its range is not looked at; bins == 0 needs no hist
    assert _spec(hist=None, bins=0, lo=1.0, hi=0.0, ws_bytes=need - 1) == EWORKSPACE
    # an empty batch is a no-op success: returns before any device work
    assert _spec(csr=_abi.GnfCsr(0, 0, 0, 0, 0, 0), cap=0, eig=None, hist=None, ws=None, ws_bytes=0) == 0
    assert _spec(csr=_abi.GnfCsr(0, 0, 0, 0, 0, 0), cap=0, eig=None, hist=None, bins=0, ws=None, ws_bytes=0) == 0


def test_python_layer_fails_loudly_without_a_hip_device():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd.graph_stats import evaluate_generated, graph_spectra, spectral_mmd
    assert gnf_amd.graph_spectra is graph_spectra and gnf_amd.spectral_mmd is spectral_mmd
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_spectra(g)
    with pytest.raises(_abi.GnfError):
        graph_spectra(g, max_nodes_per_graph=3)
    h = torch.ones(2, 200, dtype=torch.int32)
    with pytest.raises(_abi.GnfError):
        spectral_mmd(h, h)
    with pytest.raises(_abi.GnfError):
        spectral_mmd({"spectral_hist": h}, h)
    with pytest.raises(_abi.GnfError):
        evaluate_generated(g, g, spectral=True)
