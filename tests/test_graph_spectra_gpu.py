"""gnf_amd.graph_stats.graph_spectra / spectral_mmd (gnf_graph_spectra) on the MI355X against numpy.linalg.eigvalsh on the
Laplacian of tests/graph_spectra_ref.py.

Eigenvalues are held to EIG_ATOL = 1e-11 absolute.  That bound is derived, not measured: Householder tridiagonalisation and
bisection on Sturm counts are backward stable, so the computed values are the exact eigenvalues of L + E with
|E|_2 <= c n u |L|_2, u = 1.1e-16, |L|_2 <= 2, n <= 361 (the largest graph of the reference's data sets) and c a modest
constant - about 1e-12 - and LAPACK's own error has the same order; a numpy prototype of the same steps measured 4e-15 on
these cases.  Histograms are asserted EQUAL: tests/test_graph_spectra_cpu.py holds every case here at least 1e-9 away from
every bin edge, so an error of 1e-11 cannot move a count.  The worst error per case is printed before it is asserted
(measured on the MI355X: at most 3.55e-15, the 139-node ring on either route)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_graphs_ref as DR
import graph_spectra_ref as R
import graph_stats_ref as S
from helpers import graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MMD_ATOL = 1e-10   # the project's bound for the same reduction (tests/test_graph_stats_gpu.py)
SPELLINGS = ["symmetric", "one_direction", "duplicates_and_loops"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _spell(cases, how, rng=None):
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
    return graph_from_arrays(n_node, n_edge, cat(ss), cat(rr), np.zeros((off, 1), np.float32), DEV)


def _want(cases, **kw):
    return R.graph_spectra(*R.batch(cases), **kw)


def _assert_spectra(out, want, cases, what=""):
    assert out["eigenvalues"].dtype == torch.float64 and out["spectral_hist"].dtype == torch.int32
    assert out["n_node"].dtype == torch.int32 and all(v.device.type == "cuda" for v in out.values())
    eig, hist = out["eigenvalues"].cpu().numpy(), out["spectral_hist"].cpu().numpy()
    assert eig.shape == want["eigenvalues"].shape and hist.shape == want["spectral_hist"].shape
    off, worst = 0, 0.0
    for name, n, _ in cases:
        e, w = eig[off:off + n], want["eigenvalues"][off:off + n]
        err = float(np.abs(e - w).max()) if n else 0.0
        worst = max(worst, err)
        print(f"{what} {name}: n={n} max |eigenvalue - eigvalsh| = {err:.3g}")
        assert (np.diff(e) >= 0).all(), (what, name, "not ascending")
        assert err <= R.EIG_ATOL, (what, name, err)
        off += n
    print(f"{what} worst eigenvalue error {worst:.3g}")
    np.testing.assert_array_equal(hist, want["spectral_hist"], err_msg=what)
    assert hist.sum(1).tolist() == [n for _, n, _ in cases] == out["n_node"].cpu().tolist()


@pytest.fixture(scope="module")
def mixed():
    cases = R.mixed_cases()
    return {"cases": cases, "n_node": [n for _, n, _ in cases], "want": _want(cases)}


@pytest.fixture(scope="module")
def mixed_spectra(mixed):
    """graph_spectra of the mixed batch (symmetric spelling), computed once for the tests that only read it"""
    from gnf_amd.graph_stats import graph_spectra
    g = _spell(mixed["cases"], "symmetric")
    return g, graph_spectra(g)


@pytest.fixture(scope="module")
def other():
    cases = R.other_cases()
    from gnf_amd.graph_stats import graph_spectra
    g = _spell(cases, "duplicates_and_loops", np.random.default_rng(9))
    return {"cases": cases, "graph": g, "want": _want(cases), "out": graph_spectra(g)}


# ---- 1. / 2. the mixed batch, clean and messy ------------------------------------------------------------------------------
def test_mixed_batch_against_eigvalsh(mixed, mixed_spectra):
    _, out = mixed_spectra
    assert set(out) == {"eigenvalues", "spectral_hist", "n_node"}
    assert out["spectral_hist"].shape == (13, 200) and not out["spectral_hist"][0].any()
    _assert_spectra(out, mixed["want"], mixed["cases"], "mixed")
    top = out["eigenvalues"].cpu().numpy()[np.cumsum(mixed["n_node"])[10] - 1]          # the 6 x 6 grid's largest: 2, bipartite
    assert abs(top - 2.0) <= R.EIG_ATOL and out["spectral_hist"][10, 199].item() >= 1


@pytest.mark.parametrize("how", SPELLINGS[1:])
def test_messy_encodings_give_the_same_bits(mixed, mixed_spectra, how):
    from gnf_amd.graph_stats import graph_spectra
    _, clean = mixed_spectra
    out = graph_spectra(_spell(mixed["cases"], how, np.random.default_rng(7)))
    for k in ("eigenvalues", "spectral_hist", "n_node"):
        assert torch.equal(out[k], clean[k]), (how, k)


# ---- 3. routes -------------------------------------------------------------------------------------------------------------
def test_routes_agree(mixed, mixed_spectra):
    from gnf_amd.graph_stats import SPECTRA_LDS_NODES as NL, SPECTRA_SLOTS as SL, graph_spectra
    cases = R.route_cases(NL)
    want = _want(cases)
    assert [n for _, n, _ in cases] == [NL, NL + 1, NL + 60]
    # the matrices in the workspace: the bound is the largest graph
    ws = graph_spectra(_spell(cases, "one_direction"))
    _assert_spectra(ws, want, cases, "workspace")
    # the first graph alone, bounded by n_lds: the matrix in LDS
    lds = graph_spectra(_spell(cases[:1], "one_direction"), max_nodes_per_graph=NL)
    _assert_spectra(lds, _want(cases[:1]), cases[:1], "lds")
    diff = (lds["eigenvalues"] - ws["eigenvalues"][:NL]).abs().max().item()
    print(f"ring{NL}: LDS route against workspace route {diff:.3g}")
    assert diff <= R.EIG_ATOL and torch.equal(lds["spectral_hist"][0], ws["spectral_hist"][0])
    # more graphs than slots on the workspace route (forced by a bound above n_lds): every slot is used again
    reps = (SL + len(mixed["cases"]) - 1) // len(mixed["cases"]) + 1
    many = mixed["cases"] * reps
    assert len(many) > SL + len(mixed["cases"])
    out = graph_spectra(_spell(many, "one_direction"), max_nodes_per_graph=NL + 1)
    _, small = mixed_spectra                                   # the same graphs on the LDS route
    n = sum(mixed["n_node"])
    eig = out["eigenvalues"].view(reps, n)
    diff = (eig - small["eigenvalues"].unsqueeze(0)).abs().max().item()
    print(f"{len(many)} graphs in {SL} slots: workspace route against LDS route {diff:.3g}")
    assert diff <= R.EIG_ATOL
    assert torch.equal(eig, eig[:1].expand(reps, n))           # a graph's bits do not depend on its slot or turn
    assert torch.equal(out["spectral_hist"].view(reps, -1, 200), small["spectral_hist"].unsqueeze(0).expand(reps, -1, 200))


# ---- 4. other bounds -------------------------------------------------------------------------------------------------------
def test_bounds_sizes_on_the_host_and_bins(mixed, mixed_spectra):
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    from gnf_amd.graph_stats import graph_spectra
    g, first = mixed_spectra
    for kw in ({"max_nodes_per_graph": 100}, {"n_node_host": mixed["n_node"]}, {"max_nodes_per_graph": 130}):
        out = graph_spectra(g, **kw)
        for k in ("eigenvalues", "spectral_hist"):
            assert torch.equal(out[k], first[k]), (kw, k)
    one = graph_spectra(g, bins=1)
    assert one["spectral_hist"][:, 0].tolist() == mixed["n_node"] and torch.equal(one["eigenvalues"], first["eigenvalues"])
    few = graph_spectra(g, bins=7, lo=0.25, hi=1.75)             # eigenvalues on both sides of the range: clamped, none lost
    want = _want(mixed["cases"], lo=0.25, hi=1.75, bins=7)
    np.testing.assert_array_equal(few["spectral_hist"].cpu().numpy(), want["spectral_hist"])
    # bins == 0, hist == NULL through the raw entry point: eigenvalues only
    lib = _abi.lib()
    n, b = int(g.nodes.shape[0]), int(g.n_node.shape[0])
    desc = csr_desc(g, csr_of(g), node_offsets=True)
    eig = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    ws_bytes = lib.gnf_graph_spectra_workspace_bytes(b, n, 65)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _abi.check(lib.gnf_graph_spectra(C.byref(desc), 65, _abi.ptr(eig), None, 0, 0.0, 0.0, _abi.ptr(ws), ws_bytes,
                                     _abi.stream_ptr(torch.device(DEV))), "gnf_graph_spectra")
    assert torch.equal(eig, first["eigenvalues"])


# ---- 5. reproducibility and capture ----------------------------------------------------------------------------------------
def test_graph_spectra_repeats_and_replays_bitwise(mixed, mixed_spectra):
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured with
    torch.cuda.graph (one stream, no branches), replayed twice, and compared with the eager call."""
    from gnf_amd.graph_stats import graph_spectra
    g, first = mixed_spectra
    eager = graph_spectra(g, max_nodes_per_graph=65)          # (also the first launches: CSR and offsets caches)
    for k in ("eigenvalues", "spectral_hist"):
        assert torch.equal(eager[k], first[k]), k
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = graph_spectra(g, max_nodes_per_graph=65)
    for _ in range(2):
        captured["eigenvalues"].fill_(-1.0), captured["spectral_hist"].fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for k in ("eigenvalues", "spectral_hist"):
            assert torch.equal(captured[k], eager[k]), k


# ---- 6. spectral_mmd -------------------------------------------------------------------------------------------------------
def test_spectral_mmd_against_float64(mixed, mixed_spectra, other):
    from gnf_amd.graph_stats import hist_mmd, spectral_mmd
    _, a = mixed_spectra
    b = other["out"]
    _assert_spectra(b, other["want"], other["cases"], "other")
    for sigma in (1.0, 0.3):
        want = S.mmd2(mixed["want"]["spectral_hist"], other["want"]["spectral_hist"], "gaussian_tv", sigma, 1.0)
        got = spectral_mmd(a, b, sigma)
        print(f"spectral_mmd sigma={sigma}: {float(got):.17g} vs {want:.17g}")
        assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == "cuda"
        assert want > 1e-3 and abs(float(got) - want) <= MMD_ATOL
        assert torch.equal(got, spectral_mmd(a["spectral_hist"], b["spectral_hist"], sigma))      # two histogram tensors
        # hist_mmd's estimator on the same entry point, its blocks added up in another order: at most 13 x 13 kernel values
        # in [0, 1] per block, 169 * 2^-53 = 2e-14 each way before the division by the counts
        assert abs(float(got) - float(hist_mmd(a["spectral_hist"], b["spectral_hist"], "gaussian_tv", sigma, 1.0))) <= 1e-13
    assert torch.equal(spectral_mmd(a, b), spectral_mmd(a, b, 1.0))
    assert float(spectral_mmd(a, a)) == 0.0 and float(spectral_mmd(b, b["spectral_hist"], 0.3)) == 0.0
    assert float(spectral_mmd(a, {"spectral_hist": a["spectral_hist"].clone()}, 0.3)) == 0.0
    with pytest.raises(ValueError):
        spectral_mmd(a, torch.zeros(2, 200, dtype=torch.int32, device=DEV))             # no graph with nodes in a set


# ---- 7. evaluate_generated -------------------------------------------------------------------------------------------------
def test_evaluate_generated_with_spectral(mixed, mixed_spectra, other):
    from gnf_amd.graph_stats import evaluate_generated, graph_stats, hist_mmd, spectral_mmd
    g, a = mixed_spectra
    h, b = other["graph"], other["out"]
    plain = evaluate_generated(g, h)
    assert set(plain) == {"degree_mmd", "clustering_mmd"}
    sg, sh = graph_stats(g, clustering_bins=100), graph_stats(h, clustering_bins=100)      # what the call computed before
    assert torch.equal(plain["degree_mmd"], hist_mmd(sg["degree_hist"], sh["degree_hist"], "gaussian_emd", 1.0, 1.0))
    assert torch.equal(plain["clustering_mmd"], hist_mmd(sg["clustering_hist"], sh["clustering_hist"], "gaussian_emd", 0.1, 100.0))
    for k, v in S.evaluate(S.graph_stats(*R.batch(mixed["cases"])), S.graph_stats(*R.batch(other["cases"]))).items():
        assert abs(float(plain[k]) - v) <= MMD_ATOL, k
    full = evaluate_generated(g, h, spectral=True)
    assert set(full) == {"degree_mmd", "clustering_mmd", "spectral_mmd"}
    assert torch.equal(full["degree_mmd"], plain["degree_mmd"]) and torch.equal(full["clustering_mmd"], plain["clustering_mmd"])
    want = S.mmd2(mixed["want"]["spectral_hist"], other["want"]["spectral_hist"], "gaussian_tv", 1.0, 1.0)
    print(f"spectral_mmd: {float(full['spectral_mmd']):.17g} vs {want:.17g}")
    assert full["spectral_mmd"].dtype == torch.float64 and full["spectral_mmd"].dim() == 0
    assert abs(float(full["spectral_mmd"]) - want) <= MMD_ATOL and torch.equal(full["spectral_mmd"], spectral_mmd(a, b))
    assert set(evaluate_generated(g, h, True, True)) == {"degree_mmd", "clustering_mmd", "orbit_mmd", "spectral_mmd"}
    from_dicts = evaluate_generated({**sg, **a}, {**sh, **b}, spectral=True)
    assert torch.equal(from_dicts["spectral_mmd"], full["spectral_mmd"])
    with pytest.raises(ValueError):
        evaluate_generated(sg, sh, spectral=True)
    assert float(evaluate_generated(g, g, spectral=True)["spectral_mmd"]) == 0.0


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def test_errors(mixed, mixed_spectra):
    from gnf_amd import _abi
    from gnf_amd.graph_stats import SPECTRA_MAX_NODES_PER_GRAPH, graph_spectra
    g, _ = mixed_spectra
    cpu = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 1), np.float32))
    with pytest.raises(_abi.GnfError):
        graph_spectra(cpu)
    with pytest.raises(ValueError):
        graph_spectra(g, n_node_host=mixed["n_node"], max_nodes_per_graph=64)      # below the largest graph (65)
    with pytest.raises(ValueError):
        graph_spectra(g, max_nodes_per_graph=SPECTRA_MAX_NODES_PER_GRAPH + 1)
    graph_spectra(g, max_nodes_per_graph=SPECTRA_MAX_NODES_PER_GRAPH)              # the bound itself is accepted
    with pytest.raises(ValueError):
        graph_spectra(g, bins=0)
    with pytest.raises(ValueError):
        graph_spectra(g, lo=2.0, hi=2.0)


# ---- 9. after generation ---------------------------------------------------------------------------------------------------
def test_decoded_graph_needs_no_csr_build(monkeypatch):
    from gnf_amd import graphs as G
    from gnf_amd.flow import decode_graphs
    from gnf_amd.graph_stats import graph_spectra
    n_node = [1, 12, 0, 33, 20]
    z, _ = DR.clustered_embeddings(np.random.default_rng(3), n_node, 3)
    shell = graph_from_arrays(n_node, np.zeros(len(n_node), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)
    graph = decode_graphs(shell, self_loops=True)["graph"]
    s, r = graph.senders.cpu().numpy(), graph.receivers.cpu().numpy()
    assert len(s) > sum(n_node)
    want = R.graph_spectra(n_node, s, r)
    assert R.edge_margin(want["eigenvalues"]) >= R.MARGIN      # cliques: k / (k - 1), off the bin edges like every other case
    assert (want["eigenvalues"] > 1.0).sum() > 30
    cases = [(f"decoded{k}", n, None) for k, n in enumerate(n_node)]

    def boom(*a, **k):
        raise AssertionError("gnf_build_csr launched for a graph whose CSR decode_graphs seeded")
    monkeypatch.setattr(G, "build_csr_device", boom)
    _assert_spectra(graph_spectra(graph), want, cases, "decoded")
