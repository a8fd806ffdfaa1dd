"""flow.decode_graphs / gnf_adj_edges_*: everything that needs no GPU - the symbols, the host-side workspace size, the
argument validation before any launch, the no-CPU-fallback rule, the numpy helper of the GPU tests against the float64
oracle (with the margin that makes its clustered inputs rounding-proof) and the CSR cache seeding."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnf_amd import _abi
from oracle import gnf_oracle as O

import decode_graphs_ref as R

NEW_SYMBOLS = ("gnf_adj_edges_workspace_bytes", "gnf_adj_edges_count_f32", "gnf_adj_edges_fill")
P = 0x1000   # a non-null pointer that validation never dereferences


def test_symbols_are_exported_and_bound():
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        assert s in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert lib.gnf_abi_version() == 10


def test_workspace_size_is_positive_and_monotone():
    ws = _abi.lib().gnf_adj_edges_workspace_bytes
    base = ws(4, 100, 64)
    # node offsets (B + 1) int64 | bitmap [N][ceil(max / 64)] uint64 | row counts [N] int32
    assert base == 5 * 8 + 100 * 1 * 8 + 100 * 4
    assert ws(0, 0, 0) > 0
    assert ws(5, 100, 64) > base and ws(4, 101, 64) > base and ws(4, 100, 65) > base
    assert ws(4, 100, 63) <= base
    for a, b in ((1, 2), (7, 300), (300, 301)):
        assert ws(a, 50, 40) <= ws(b, 50, 40) and ws(3, a, 40) <= ws(3, b, 40) and ws(3, 50, a) <= ws(3, 50, b)
    assert ws(-1, 10, 10) == 0


def _count(z=P, ld=8, d=8, n_node=P, b=3, n=40, cap=20, rowptr=P, n_edge=P, total=P, ws=P, ws_bytes=1 << 20):
    return _abi.lib().gnf_adj_edges_count_f32(z, ld, d, n_node, b, n, cap, 0.5, 0, rowptr, n_edge, total, ws, ws_bytes, None)


def _fill(b=3, n=40, cap=20, rowptr=P, ecap=100, s=P, r=P, ws=P, ws_bytes=1 << 20):
    return _abi.lib().gnf_adj_edges_fill(b, n, cap, rowptr, ecap, s, r, ws, ws_bytes, None)


def test_argument_validation_without_a_gpu():
    ESHAPE, EINVAL, EWORKSPACE = -2, -1, -3
    assert _count(d=0) == ESHAPE
    assert _count(ld=7) == ESHAPE
    assert _count(b=-1) == ESHAPE and _count(n=-1) == ESHAPE and _count(cap=-1) == ESHAPE
    assert _count(n=1 << 20, cap=1 << 12) == ESHAPE          # 2^32 possible edges: the ids are int32
    assert "int32" in _abi.lib().gnf_last_error().decode()
    assert _count(n=40, cap=0) == ESHAPE
    for name in ("z", "n_node", "rowptr", "n_edge", "total", "ws"):
        assert _count(**{name: None}) == EINVAL, name
    need = _abi.lib().gnf_adj_edges_workspace_bytes(3, 40, 20)
    assert _count(ws_bytes=need - 1) == EWORKSPACE
    assert "workspace" in _abi.lib().gnf_last_error().decode()
    assert _fill(b=-1) == ESHAPE and _fill(n=-1) == ESHAPE and _fill(cap=-1) == ESHAPE and _fill(ecap=-1) == ESHAPE
    assert _fill(n=1 << 20, cap=1 << 12) == ESHAPE
    for name in ("rowptr", "s", "r", "ws"):
        assert _fill(**{name: None}) == EINVAL, name
    assert _fill(ws_bytes=need - 1) == EWORKSPACE
    assert _fill(ecap=0, s=None, r=None) == 0                # nothing to write: returns before any launch


def test_decode_graphs_fails_loudly_without_a_hip_device():
    from helpers import graph_from_arrays
    from gnf_amd.flow import decode_graphs, generate_graphs
    g = graph_from_arrays([2], [0], [], [], np.zeros((2, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        decode_graphs(g)
    with pytest.raises(NotImplementedError):
        decode_graphs(g, distance_fn=lambda *a: None)
    assert callable(generate_graphs)


N_NODE = [1, 63, 64, 65, 130, 0, 17]


@pytest.mark.parametrize("d", [1, 3, 200])
def test_helper_matches_the_oracle_on_clustered_inputs(d):
    """The condition of the GPU test's float64 case, checked on the reference alone: inside a cluster P >= 0.999, across
    clusters P <= 1e-12, so thresholds 0.1 / 0.5 / 0.9 all give the disjoint cliques - from the closed form and from
    oracle.pred_adj_blocks + numpy.nonzero alike."""
    z, lab = R.clustered_embeddings(np.random.default_rng(d), N_NODE, d)
    assert z.dtype == np.float32 and z.shape == (sum(N_NODE), d)
    with np.errstate(over="ignore"):      # exp(10 (d2 / sqrt(D) - 1)) overflows to inf for far clusters: P = 0 exactly
        blocks = O.pred_adj_blocks(z, N_NODE)
    off = 0
    for n, b in zip(N_NODE, blocks):
        same = lab[off:off + n, None] == lab[None, off:off + n]
        offdiag = ~np.eye(n, dtype=bool)
        if (same & offdiag).any():
            assert b[same & offdiag].min() >= 0.999
        if (~same).any():
            assert b[~same].max() <= 1e-12
        zz = z[off:off + n].astype(np.float64)
        d2 = ((zz[:, None, :] - zz[None, :, :]) ** 2).sum(-1) / np.sqrt(d)
        assert d2[same].max(initial=0.0) <= R.INSIDE_MAX and d2[~same].min(initial=np.inf) >= R.ACROSS_MIN
        off += n
    for loops in (False, True):
        want = R.edges_from_blocks(R.clique_blocks(N_NODE, lab), 0.5, loops)
        for t in (0.1, 0.5, 0.9):
            got = R.edges_from_blocks(blocks, t, loops)
            for k in ("senders", "receivers", "rowptr", "n_edge"):
                np.testing.assert_array_equal(got[k], want[k])
            # ... and numpy.nonzero on the dense block-diagonal matrix, spelled out
            s, r, o = [], [], 0
            for n, b in zip(N_NODE, blocks):
                m = b > t
                m[np.eye(n, dtype=bool)] = loops
                i, j = np.nonzero(m)
                r.append(i + o), s.append(j + o)
                o += n
            np.testing.assert_array_equal(got["senders"], np.concatenate(s))
            np.testing.assert_array_equal(got["receivers"], np.concatenate(r))
            assert got["total"] == len(got["senders"]) == got["n_edge"].sum() == got["rowptr"][-1]
            # (rowptr, senders) is the receiver-sorted CSR of the list, and its transpose
            from gnf_amd.graphs import build_csr_host
            for a, b_ in ((got["senders"], got["receivers"]), (got["receivers"], got["senders"])):
                rp, col = build_csr_host(a, b_, sum(N_NODE))
                np.testing.assert_array_equal(rp, got["rowptr"])
                np.testing.assert_array_equal(col, got["senders"])


def test_seed_csr_cache_is_what_csr_of_returns(monkeypatch):
    from gnf_amd import graphs as G
    from helpers import graph_from_arrays
    G.clear_csr_cache()
    g = graph_from_arrays([3], [4], [0, 1, 2, 0], [0, 1, 2, 1], np.zeros((3, 2), np.float32))
    rowptr = torch.tensor([0, 1, 3, 4], dtype=torch.int32)
    csr = G.Csr(rowptr, g.senders, 3, 4)

    def boom(*a, **k):
        raise AssertionError("csr_of called the library for a seeded graph")
    monkeypatch.setattr(G, "build_csr_device", boom)
    assert G.seed_csr_cache(g, csr) is csr
    assert G.csr_of(g) is csr
    assert G.csr_of(g.replace(nodes=torch.ones(3, 2))) is csr        # keyed on the index tensors, as before
    with pytest.raises(AssertionError):
        G.csr_of(g, by_sender=True)                                   # the other orientation was not seeded
    other = G.Csr(rowptr, g.receivers, 3, 4)
    G.seed_csr_cache(g, other, by_sender=True)
    assert G.csr_of(g, by_sender=True) is other and G.csr_of(g) is csr
    G.clear_csr_cache()
