"""The random graph models without a device (include/gnf_random_graphs.h, gnf_amd.random_graphs): header, exports and binding in
step; every rejection with its code and text before any launch; the workspace is the decoder's; the numpy twin against the
pure-Python restatement, integer for integer; known answers (every pair, only the loops, the Barabasi-Albert edge count, degrees,
connectivity and fallback); first_graph splits; the densities at fixed seeds against derived bounds; the baseline fit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import random_graphs_ref as RR
from gnf_amd import _abi, random_graphs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnf_random_graph_edges_count",)
GNF_EINVAL, GNF_ESHAPE, GNF_EWORKSPACE, GNF_EUNSUPPORTED = -1, -2, -3, -5
P = 1 << 20   # a made-up non-null pointer: every call below fails before any launch, nothing is dereferenced
SIZES = [1, 2, 63, 64, 65, 0, 129]          # both sides of a bitmap word's edge, the empty graph mid-batch
KEYS = ("senders", "receivers", "rowptr", "n_edge")
NEXT_TO_ZERO = 2.0 ** -32                   # thr = 1: only a draw of 0 is an edge


def test_symbols_are_exported_and_bound():
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert main.index('#include "gnf_synthetic.h"') < main.index('#include "gnf_random_graphs.h"')
    assert re.search(r"^#define GNF_ABI_VERSION 10$", main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_random_graphs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.RANDOM_GRAPH_SYMBOLS)
    for name in dir(_abi):
        if name.endswith("_SYMBOLS") and name != "RANDOM_GRAPH_SYMBOLS":
            assert not set(_abi.RANDOM_GRAPH_SYMBOLS) & set(getattr(_abi, name))
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    fields = re.search(r"typedef struct GnfRandomGraphSpec \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"([a-z_]+);", fields) == [f[0] for f in _abi.GnfRandomGraphSpec._fields_]
    assert re.search(r"GNF_RG_PLANTED = 0, GNF_RG_BARABASI_ALBERT = 1", text)
    assert (_abi.GNF_RG_PLANTED, _abi.GNF_RG_BARABASI_ALBERT) == (0, 1)
    for name in ("GNF_RG_BA_DRAWS", "GNF_RG_MAX_M", "GNF_RG_BA_TABLE_MAX"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_abi, name)
    assert int(re.search(r"#define GNF_RG_BA_SEED_XOR (0x[0-9A-F]+)ull", text).group(1), 16) == _abi.GNF_RG_BA_SEED_XOR == RR.BA_SEED_XOR
    assert RR.BA_DRAWS == _abi.GNF_RG_BA_DRAWS


def _spec(model=0, thr_in=P, thr_out=None, block=None, n_blocks=1, m_dev=P, max_m=4):
    sp = _abi.GnfRandomGraphSpec()
    sp.seed, sp.seed_dev, sp.first_graph, sp.model, sp.self_loops = 1, None, 0, model, 0
    sp.thr_in, sp.thr_out, sp.block, sp.n_blocks, sp.m_dev, sp.max_m = thr_in, thr_out, block, n_blocks, m_dev, max_m
    return sp


def _count(spec=None, null_spec=False, n_node=P, b=4, n=10, cap=8, rowptr=P, n_edge=P, total=P, ws=P, ws_bytes=None):
    lib = _abi.lib()
    spec = _spec() if spec is None else spec
    if ws_bytes is None:
        ws_bytes = max(lib.gnf_adj_edges_workspace_bytes(max(b, 0), max(n, 0), max(cap, 0)), 8)
    rc = lib.gnf_random_graph_edges_count(None if null_spec else C.byref(spec), n_node, b, n, cap, rowptr, n_edge, total, ws,
                                          ws_bytes, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def test_rejections_come_with_their_code_and_text():
    need = _abi.lib().gnf_adj_edges_workspace_bytes(4, 10, 8)
    bad = [(dict(null_spec=True), GNF_EINVAL), (dict(rowptr=None), GNF_EINVAL), (dict(total=None), GNF_EINVAL),
           (dict(n_edge=None), GNF_EINVAL), (dict(n_node=None), GNF_EINVAL), (dict(ws=None), GNF_EINVAL),
           (dict(spec=_spec(thr_in=None)), GNF_EINVAL), (dict(spec=_spec(model=1, m_dev=None)), GNF_EINVAL),
           (dict(spec=_spec(model=2)), GNF_EINVAL), (dict(spec=_spec(model=-1)), GNF_EINVAL),
           (dict(b=-1), GNF_ESHAPE), (dict(n=-1), GNF_ESHAPE), (dict(cap=-1), GNF_ESHAPE), (dict(cap=0), GNF_ESHAPE),
           (dict(b=2 ** 31), GNF_ESHAPE), (dict(n=2 ** 20, cap=2 ** 12), GNF_ESHAPE),
           (dict(spec=_spec(n_blocks=0)), GNF_ESHAPE), (dict(spec=_spec(n_blocks=-3)), GNF_ESHAPE),
           (dict(spec=_spec(model=1, max_m=0)), GNF_ESHAPE), (dict(spec=_spec(model=1, max_m=65)), GNF_ESHAPE),
           (dict(ws_bytes=need - 1), GNF_EWORKSPACE), (dict(ws_bytes=0), GNF_EWORKSPACE),
           # the targets table: 32768 entries, and one more word per node inside 160 KB
           (dict(spec=_spec(model=1, max_m=64), n=1024, cap=513), GNF_EUNSUPPORTED),
           (dict(spec=_spec(model=1, max_m=1), n=40000, cap=20480), GNF_EUNSUPPORTED)]
    for kw, code in bad:
        rc, msg = _count(**kw)
        assert rc == code and msg.startswith("gnf_random_graph_edges_count"), (kw, rc, msg)
    assert "workspace" in _count(ws_bytes=0)[1] and "null spec" in _count(null_spec=True)[1] and "n_nodes=-1" in _count(n=-1)[1]
    assert "thr_in" in _count(spec=_spec(thr_in=None))[1] and "m_dev" in _count(spec=_spec(model=1, m_dev=None))[1]
    assert "model=2" in _count(spec=_spec(model=2))[1] and "n_blocks=0" in _count(spec=_spec(n_blocks=0))[1]
    assert "max_m=65" in _count(spec=_spec(model=1, max_m=65))[1]
    # block labels make n_blocks irrelevant; what the other model needs is not asked for: past the checks, these would launch,
    # so only the refusals that come later in the chain show that the earlier rules let them through
    assert _count(spec=_spec(block=P, n_blocks=0), ws_bytes=0)[0] == GNF_EWORKSPACE
    assert _count(spec=_spec(model=1, thr_in=None, n_blocks=0), ws_bytes=0)[0] == GNF_EWORKSPACE
    assert _count(spec=_spec(model=0, m_dev=None, max_m=0), ws_bytes=0)[0] == GNF_EWORKSPACE
    assert _count(spec=_spec(model=1, max_m=64), n=1024, cap=512, ws_bytes=0)[0] == GNF_EWORKSPACE   # exactly 32768 entries


def test_the_workspace_is_the_decoders():
    # the random-graph call has no size function of its own: the header names gnf_adj_edges_workspace_bytes, and the smallest
    # workspace it accepts is that function's value
    raw = open(os.path.join(ROOT, "include", "gnf_random_graphs.h")).read()
    assert "gnf_adj_edges_workspace_bytes(n_graphs, n_nodes, max_nodes_per_graph)" in raw
    f = _abi.lib().gnf_adj_edges_workspace_bytes
    for b, n, cap in ((1, 1, 1), (4, 10, 8), (7, 324, 129), (32, 11552, 361), (3, 200, 65)):
        need = f(b, n, cap)
        assert need == (((b + 1) * 8 + n * ((cap + 63) // 64) * 8 + n * 4 + 7) // 8) * 8
        for model in (0, 1):
            rc, msg = _count(spec=_spec(model=model), b=b, n=n, cap=cap, ws_bytes=need - 1)
            assert rc == GNF_EWORKSPACE and f"< {need} bytes" in msg, msg


def _same(h, r):
    for k in KEYS:
        assert h[k].dtype == np.int32 and h[k].tolist() == r[k], k
    assert h["total"] == r["total"] and h["fallbacks"] == r["fallbacks"]


@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("p", [0.0, NEXT_TO_ZERO, 0.3, 1.0])
def test_erdos_renyi_twin_equals_the_restatement(p, self_loops):
    b = len(SIZES)
    h = G.random_graphs_host("erdos_renyi", SIZES, G.thresholds(p, b), seed=12345, self_loops=self_loops)
    r = RR.batch("planted", SIZES, [RR.threshold(p)] * b, seed=12345, self_loops=self_loops)
    _same(h, r)
    pairs = sum(n * (n - 1) // 2 for n in SIZES)
    loops = sum(SIZES) if self_loops else 0
    if p == 1.0:
        assert h["total"] == 2 * pairs + loops                    # every pair
        assert all(len(s) == n * (n - 1) // 2 for s, n in zip(r["edge_sets"], SIZES))
    if p == 0.0:
        assert h["total"] == loops                                 # exactly the loops
        assert np.array_equal(h["senders"], h["receivers"]) and h["senders"].tolist() == list(range(loops))
    if p == NEXT_TO_ZERO:
        assert h["total"] - loops <= 2                             # 13 000 pairs at 2^-32 each
    if p == 0.3:
        assert 0 < h["total"] - loops < 2 * pairs


@pytest.mark.parametrize("n_blocks", [1, 2, 3])
def test_planted_twin_equals_the_restatement(n_blocks):
    b = len(SIZES)
    p_in, p_out = np.linspace(0.2, 0.8, b), np.linspace(0.3, 0.0, b)
    h = G.random_graphs_host("planted_partition", SIZES, G.thresholds(p_in, b), G.thresholds(p_out, b), n_blocks=n_blocks,
                             seed=2 ** 63 + 5, first_graph=9, self_loops=True)
    r = RR.batch("planted", SIZES, [RR.threshold(p) for p in p_in], [RR.threshold(p) for p in p_out], n_blocks=n_blocks,
                 seed=2 ** 63 + 5, first_graph=9, self_loops=True)
    _same(h, r)
    if n_blocks == 1:   # one block: thr_out is never looked at - G(n, p_in)
        er = G.random_graphs_host("erdos_renyi", SIZES, G.thresholds(p_in, b), seed=2 ** 63 + 5, first_graph=9, self_loops=True)
        assert all(np.array_equal(er[k], h[k]) for k in KEYS)


def test_planted_twin_with_explicit_blocks_equals_the_restatement():
    b, n = len(SIZES), sum(SIZES)
    blocks = (np.arange(n) * 7 % 5).astype(np.int32)               # interleaved labels, nothing like the default
    h = G.random_graphs_host("planted_partition", SIZES, G.thresholds(0.9, b), G.thresholds(0.05, b), blocks=blocks, seed=3)
    r = RR.batch("planted", SIZES, [RR.threshold(0.9)] * b, [RR.threshold(0.05)] * b, blocks=blocks.tolist(), seed=3)
    _same(h, r)
    other = G.random_graphs_host("planted_partition", SIZES, G.thresholds(0.9, b), G.thresholds(0.05, b), n_blocks=5, seed=3)
    assert other["total"] != h["total"]


def _components(n, edges):
    root = list(range(n))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v
    for u, v in edges:
        root[find(u)] = find(v)
    return len({find(v) for v in range(n)})


@pytest.mark.parametrize("m", [1, 2, 40, 64])
def test_barabasi_albert_twin_equals_the_restatement(m):
    b = len(SIZES)
    h = G.random_graphs_host("barabasi_albert", SIZES, [m] * b, seed=12345, self_loops=(m == 2))
    r = RR.batch("ba", SIZES, [m] * b, seed=12345, self_loops=(m == 2))
    _same(h, r)
    for n, edges in zip(SIZES, r["edge_sets"]):
        if n <= m:
            assert not edges                                        # n <= m: no edges
            continue
        assert len(edges) == m * (n - m)
        degree = [0] * n
        for u, v in edges:
            assert u < v
            degree[u] += 1
            degree[v] += 1
        assert all(degree[t] >= m for t in range(m, n)) and _components(n, edges) == 1
    # m out of range is clamped: 0 -> 1, 99 -> max_m
    lo = G.random_graphs_host("barabasi_albert", [20], [0], seed=1)
    assert all(np.array_equal(lo[k], G.random_graphs_host("barabasi_albert", [20], [1], seed=1)[k]) for k in KEYS)
    hi = G.random_graphs_host("barabasi_albert", [20], [99], seed=1, max_m=5)
    assert all(np.array_equal(hi[k], G.random_graphs_host("barabasi_albert", [20], [5], seed=1)[k]) for k in KEYS)


@pytest.mark.parametrize("n,m,want", [(44, 40, [1, 1, 2, 1]), (70, 64, [5, 5, 5, 5])])
def test_barabasi_albert_fallback(n, m, want):
    r = RR.batch("ba", [n] * 4, [m] * 4, seed=12345)
    assert all(f > 0 for f in r["fallbacks"]), r["fallbacks"]      # the fallback IS taken: the comparison below is not vacuous
    assert r["fallbacks"] == want                                   # (the figures of the rule's first prototype)
    h = G.random_graphs_host("barabasi_albert", [n] * 4, [m] * 4, seed=12345)
    _same(h, r)
    for edges in r["edge_sets"]:
        assert len(edges) == m * (n - m) and _components(n, edges) == 1
    # where the header says no fallback is met, none is, and few draws are looked at
    for nn, mm in ((200, 16), (130, 8), (65, 4)):
        _, fallbacks, most = RR.ba_targets(nn, mm, 0, 12345)
        assert fallbacks == 0 and most <= 104


def test_first_graph_splits_a_batch():
    sizes = [30, 65, 7, 64]
    for model, par, kw in (("erdos_renyi", G.thresholds([0.1, 0.5, 0.9, 0.3], 4), {}),
                           ("planted_partition", G.thresholds(0.7, 4), dict(thr_out=G.thresholds(0.1, 4), n_blocks=2)),
                           ("barabasi_albert", np.asarray([3, 1, 2, 40]), {})):
        whole = G.random_graphs_host(model, sizes, par, seed=5, **kw)
        kw_a = {k: (v[:2] if k == "thr_out" else v) for k, v in kw.items()}
        kw_b = {k: (v[2:] if k == "thr_out" else v) for k, v in kw.items()}
        a = G.random_graphs_host(model, sizes[:2], par[:2], seed=5, first_graph=0, **kw_a)
        c = G.random_graphs_host(model, sizes[2:], par[2:], seed=5, first_graph=2, **kw_b)
        assert whole["n_edge"].tolist() == a["n_edge"].tolist() + c["n_edge"].tolist()
        assert np.array_equal(whole["senders"], np.concatenate([a["senders"], c["senders"] + 95]))
        assert np.array_equal(whole["receivers"], np.concatenate([a["receivers"], c["receivers"] + 95]))
        shifted = G.random_graphs_host(model, sizes[2:], par[2:], seed=5, first_graph=0, **kw_b)
        assert not np.array_equal(shifted["senders"], c["senders"])


def test_edge_counts_are_binomial():
    """64 graphs of 200 nodes.  Each of M pairs is an edge with probability thr / 2^32 independently (distinct hash inputs), so
    the edge count is Binomial(M, p) with sigma = sqrt(M p (1 - p)); the bound is 5 sigma."""
    b, n = 64, 200
    h = G.random_graphs_host("erdos_renyi", [n] * b, G.thresholds(0.1, b), seed=12345)
    pairs = b * n * (n - 1) // 2
    sigma = math.sqrt(pairs * 0.1 * 0.9)
    assert abs(h["total"] // 2 - pairs * 0.1) <= 5 * sigma, (h["total"] // 2, pairs * 0.1, sigma)
    # planted, two blocks of 100: intra- and inter-block pairs separately
    p_in, p_out = 0.3, 0.05
    h = G.random_graphs_host("planted_partition", [n] * b, G.thresholds(p_in, b), G.thresholds(p_out, b), n_blocks=2, seed=12345)
    s, r = h["senders"] % n, h["receivers"] % n
    upper = s < r
    same = (s * 2 // n) == (r * 2 // n)
    intra, inter = int((upper & same).sum()), int((upper & ~same).sum())
    m_in, m_out = b * 2 * (100 * 99 // 2), b * 100 * 100
    assert abs(intra - m_in * p_in) <= 5 * math.sqrt(m_in * p_in * (1 - p_in)), (intra, m_in * p_in)
    assert abs(inter - m_out * p_out) <= 5 * math.sqrt(m_out * p_out * (1 - p_out)), (inter, m_out * p_out)


def test_fit_params_arithmetic():
    #                      K4  path of 3  one node  empty  star of 5  10 nodes 22 edges   200 nodes dense
    n_node = torch.tensor([4, 3, 1, 0, 5, 10, 200])
    n_edges = torch.tensor([6, 2, 0, 0, 4, 22, 19000])
    p = G.fit_params(n_edges, n_node, "erdos_renyi")
    assert p.dtype == torch.float64 and p.tolist() == [1.0, 2 / 3, 0.0, 0.0, 0.4, 22 / 45, 19000 / 19900]
    m = G.fit_params(n_edges, n_node, "barabasi_albert")
    # round(E / n) = floor(E / n + 1/2): 1.5 -> 2, 0.67 -> 1, 0 -> (clamped) 1, 0.8 -> 1, 2.2 -> 2, 95 -> min(64, n - 1) = 64
    assert m.dtype == torch.int32 and m.tolist() == [2, 1, 1, 1, 1, 2, 64]
    assert G.fit_params(torch.tensor([5]), torch.tensor([3]), "barabasi_albert").tolist() == [2]   # min(.., n - 1)
    with pytest.raises(ValueError):
        G.fit_params(n_edges, n_node, "planted_partition")


def test_the_generators_on_the_cpu_are_the_twin():
    out = G.erdos_renyi(SIZES, 0.3, seed=12345, device="cpu")
    h = G.random_graphs_host("erdos_renyi", SIZES, G.thresholds(0.3, len(SIZES)), seed=12345)
    g = out["graph"]
    assert np.array_equal(g.senders.numpy(), h["senders"]) and np.array_equal(g.receivers.numpy(), h["receivers"])
    assert np.array_equal(g.n_edge.numpy(), h["n_edge"]) and np.array_equal(out["csr"].rowptr.numpy(), h["rowptr"])
    assert int(out["total_edges"]) == h["total"] and g.nodes.shape == (sum(SIZES), 1) and not g.nodes.any()
    assert g.senders.dtype == torch.int32 and g.n_node.tolist() == SIZES and g.edges.shape == (h["total"],)
    out = G.barabasi_albert([30, 12], [3, 40], seed=4, self_loops=True, device="cpu", edge_capacity=50)
    h = G.random_graphs_host("barabasi_albert", [30, 12], [3, 40], seed=4, self_loops=True)
    assert out["graph"].senders.shape == (50,) and np.array_equal(out["graph"].senders.numpy(), h["senders"][:50])
    assert int(out["total_edges"]) == h["total"] == 2 * 3 * 27 + 42
    out = G.planted_partition([40], 0.8, 0.1, n_blocks=4, seed=1, device="cpu", nodes=torch.ones(40, 3))
    h = G.random_graphs_host("planted_partition", [40], G.thresholds(0.8, 1), G.thresholds(0.1, 1), n_blocks=4, seed=1)
    assert np.array_equal(out["graph"].senders.numpy(), h["senders"]) and out["graph"].nodes.shape == (40, 3)
    with pytest.raises(ValueError):
        G.erdos_renyi([4], 1.5, device="cpu")
