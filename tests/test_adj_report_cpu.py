"""gnf_amd.adj_loss.reconstruction_report / gnf_adj_report_*: everything that needs no GPU - the float64 restatement the GPU
tests compare against (classes, edge order, counts on a hand-made batch; the quantile rule against np.quantile), the conditions
on every batch the GPU tests use, the symbols, the host-side workspace size, the argument validation before any launch and the
Python layer's argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gnf_amd import _abi

import adj_loss_ref as R
import adj_report_ref as A

NEW_SYMBOLS = ("gnf_adj_report_workspace_bytes", "gnf_adj_report_count_f32", "gnf_adj_report_fill", "gnf_score_select_f32")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_classes_order_and_counts_on_a_hand_made_batch():
    # graph 0: nodes 0, 1 close together, 2 far away; graph 1: nodes 3, 4 close.  scaled_hacky at D = 2: p > 0.5 iff d2 < sqrt(2)
    z = np.array([[0.0, 0.0], [0.1, 0.0], [5.0, 5.0], [0.0, 0.0], [0.2, 0.2]], np.float32)
    # true edges (sender -> receiver): 0 -> 1 twice (correct), 2 -> 0 (false negative), a self loop and an edge into the other
    # graph (both ignored); 1 -> 0 and both directions of 3 - 4 are predicted without being true (false positives)
    s, r = np.array([0, 0, 2, 1, 1]), np.array([1, 1, 0, 1, 3])
    rep = A.report(z, [3, 2], s, r)
    assert rep["receivers"].tolist() == [0, 0, 1, 3, 4] and rep["senders"].tolist() == [1, 2, 0, 4, 3]
    assert rep["cls"].tolist() == [2, 3, 1, 2, 2]
    assert rep["rowptr"].tolist() == [0, 2, 3, 3, 4, 5] and rep["n_edge"].tolist() == [3, 2]
    assert rep["class_pairs"].tolist() == [[1, 1, 1], [0, 2, 0]] and rep["totals"].tolist() == [5, 1, 3, 1]
    assert rep["score"][1] < 1e-100 and rep["score"][0] == rep["score"][2] > 0.99   # d2 is symmetric
    ts, tr = A.true_edges([3, 2], s, r)
    assert ts.tolist() == [2, 0] and tr.tolist() == [0, 1]                       # receivers ascending, duplicates once
    keep = np.isin(rep["cls"], (1, 3))
    assert rep["senders"][keep].tolist() == ts.tolist() and rep["receivers"][keep].tolist() == tr.tolist()
    # class_pairs[:, 1:] are binary_loss' ordered-pair counts
    ref = R.binary_loss(z, [3, 2], s, r)
    assert ref["fp"].tolist() == rep["class_pairs"][:, 1].tolist() and ref["fn"].tolist() == rep["class_pairs"][:, 2].tolist()


def test_quantile_rule_equals_numpy_quantile():
    """order statistics + the host's two-operation interpolation against np.quantile(..., method="linear") on the same float64
    values.  Both evaluate a + f (b - a) (numpy as a lerp that switches to b - (b - a) (1 - f) for f >= 0.5) in float64: the
    difference, the product and the sum round once each - 3 roundings relative to quantities of at most max(|a|, |b|) - and
    numpy's form has a fourth in 1 - f: |host - numpy| <= (3 + 4) 2^-53 max(|a|, |b|), rounded up to 8."""
    rng = np.random.default_rng(5)
    qs = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0)
    for n in (1, 2, 3, 4, 5, 10, 257, 1000):
        x = rng.random(n).astype(np.float32)
        x[: n // 3] = x[0]                                                       # ties
        stat, cnt = A.order_stats(x, qs)
        assert cnt == n
        got = A.interpolate(stat, cnt, qs)
        want = np.quantile(x.astype(np.float64), qs)
        bound = 8.0 * 2.0 ** -53 * np.abs(stat.astype(np.float64)).max(1)
        assert (np.abs(got - want) <= bound).all(), (n, got - want)
        assert got[0] == x.min() and got[-1] == x.max()                          # q = 0 and q = 1 are exact
    stat, cnt = A.order_stats(np.zeros(0, np.float32), qs)
    assert cnt == 0 and np.isnan(stat).all() and np.isnan(A.interpolate(stat, cnt, qs)).all()
    # the order is that of the bit patterns: NaN sorts last, so only q = 1 sees it
    stat, cnt = A.order_stats(np.array([0.5, np.nan, 0.25], np.float32), (0.0, 0.5, 1.0))
    assert stat[0].tolist() == [0.25, 0.5] and stat[1, 0] == 0.5 and np.isnan(stat[1, 1]) and np.isnan(stat[2]).all()


def test_segment_stats_cover_every_entry_once():
    d, dist, sym, gs = A.BATCHES[1]
    _, z, (_, s, r) = A.batch(d, dist, sym, gs)
    rep = A.report(z, R.SIZES, s, r, dist)
    score = rep["score"].astype(np.float32)
    off = np.concatenate([[0], np.cumsum(R.SIZES)])
    stat_g, count_g = A.segment_stats(score, rep["cls"], rep["rowptr"], off, A.QUANTILES)
    stat_b, count_b = A.segment_stats(score, rep["cls"], rep["rowptr"], [0, off[-1]], A.QUANTILES)
    assert count_g.sum(0).tolist() == count_b[0].tolist() == rep["totals"][2:].tolist()
    assert count_g.tolist() == rep["class_pairs"][:, 1:].tolist()
    for c in (0, 1):
        x = score[rep["cls"] == c + 2]
        assert stat_b[0, c, 0, 0] == x.min() == np.nanmin(stat_g[:, c, 0, 0])
        assert stat_b[0, c, -1, 1] == x.max() == np.nanmax(stat_g[:, c, -1, 1])


# ---- the conditions on the GPU tests' inputs -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dist,sym,gs", A.BATCHES)
def test_gpu_batches_have_margin_all_classes_and_a_select_across_a_histogram_stride(d, dist, sym, gs):
    seed, z, (n_edge, s, r) = A.batch(d, dist, sym, gs)
    assert seed is not None, f"D={d}: no seed in range(16) keeps every pair 2 delta from the kinks"
    assert z.dtype == np.float32 and z.shape == (198, d) and int(n_edge.sum()) == len(s) == len(r)
    assert R.margin_ok(R.graph_blocks(z, R.SIZES, s, r, dist), d, dist)
    rep = A.report(z, R.SIZES, s, r, dist)
    print(f"D={d} {dist} symmetric={sym}: seed {seed}, totals {rep['totals'].tolist()}")
    assert (rep["totals"][1:] > 0).all()                                         # all three classes occur
    cp = rep["class_pairs"]
    assert ((cp[:, 1] > 256) & (cp[:, 2] > 256)).any()                           # one graph's select crosses a 256-entry stride
    assert cp[0].tolist() == cp[1].tolist() == [0, 0, 0]                         # the 1-node and the empty graph
    if sym:   # both directions of every true edge: the list is symmetric
        fwd = set(zip(rep["senders"].tolist(), rep["receivers"].tolist()))
        assert fwd == {(b, a) for a, b in fwd}
    # equal scores occur (duplicate rows), so the select meets ties
    assert len(np.unique(rep["score"].astype(np.float32))) < len(rep["score"])


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_adj_report.h (included by gnf.h), the library's exports and _abi.ADJ_REPORT_SYMBOLS are in step"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_adj_report.h"$', main, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_adj_report.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.ADJ_REPORT_SYMBOLS)
    for table in (_abi.EXPORTED_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.DISTANCE_SYMBOLS, _abi.RANDOM_GRAPH_SYMBOLS):
        assert not set(_abi.ADJ_REPORT_SYMBOLS) & set(table)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    assert _abi.GNF_SELECT_MAX_Q == 16 and re.search(r"#define GNF_SELECT_MAX_Q 16\b", text)


def test_workspace_size_is_a_host_computation_and_monotone():
    ws = _abi.lib().gnf_adj_report_workspace_bytes
    # node offsets int64 [B + 1] | true and pred words uint64 [N][ceil(max / 64)] each | row count int32 [N] | class counts [3][N]
    assert ws(4, 100, 64) == 5 * 8 + 2 * 100 * 1 * 8 + 100 * 4 + 3 * 100 * 4
    assert ws(4, 100, 65) == 5 * 8 + 2 * 100 * 2 * 8 + 100 * 4 + 3 * 100 * 4
    assert ws(0, 0, 0) == 8 and ws(4, 101, 64) % 8 == 0 and ws(4, 101, 64) > ws(4, 100, 64) and ws(4, 100, 63) <= ws(4, 100, 64)
    for a, b in ((1, 2), (7, 300), (300, 301), (0, 65536)):
        assert ws(a, 50, 40) <= ws(b, 50, 40) and ws(3, a, 40) <= ws(3, b, 40) and ws(3, 50, a) <= ws(3, 50, b)
    assert ws(-1, 10, 10) == 0 and ws(3, -1, 10) == 0 and ws(3, 10, -1) == 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _dist():
    return _abi.GnfDistance(10.0, 1.0, 1, None)


def _count(csr=None, dist=True, z=P, ld=8, d=8, cap=20, thr=0.5, rowptr=P, n_edge=P, pairs=P, totals=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_adj_report_count_f32(C.byref(csr), C.byref(_dist()) if dist else None, z, ld, d, cap, thr, rowptr,
                                               n_edge, pairs, totals, ws, ws_bytes, None)


def _fill(dist=True, z=P, ld=8, d=8, b=3, n=40, cap=20, rowptr=P, ecap=50, senders=P, receivers=P, cls=P, score=P, ws=P,
          ws_bytes=1 << 20):
    return _abi.lib().gnf_adj_report_fill(C.byref(_dist()) if dist else None, z, ld, d, b, n, cap, rowptr, ecap, senders,
                                          receivers, cls, score, ws, ws_bytes, None)


def _select(score=P, cls=P, rowptr=P, seg=P, n_seg=2, n=40, ecap=50, q=(0.5,), nq=None, stat=P, count=P):
    arr = (C.c_double * max(len(q), 1))(*q) if q is not None else None
    return _abi.lib().gnf_score_select_f32(score, cls, rowptr, seg, n_seg, n, ecap, arr, len(q or ()) if nq is None else nq,
                                           stat, count, None)


def test_validation_without_a_gpu():
    """every documented argument error, on fake pointers: a call that passed every check would launch on them, so each call
    here fails one (GNF_EWORKSPACE, the last check of count and fill, shows which values pass the ones before it)"""
    lib = _abi.lib()
    err = lambda: lib.gnf_last_error().decode()
    # ---- count
    assert _count(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _count(csr=_csr(b=0)) == EINVAL and _count(dist=False) == EINVAL and "dist" in err()
    assert lib.gnf_adj_report_count_f32(None, C.byref(_dist()), P, 8, 8, 20, 0.5, P, P, P, P, P, 1 << 20, None) == EINVAL
    for name in ("z", "rowptr", "n_edge", "pairs", "totals", "ws"):
        assert _count(**{name: None}) == EINVAL, name
    assert _count(csr=_csr(rowptr=None)) == EINVAL and _count(csr=_csr(col=None)) == EINVAL
    assert _count(d=0) == ESHAPE and _count(d=-3) == ESHAPE and _count(ld=7) == ESHAPE and "ld" in err()
    assert _count(csr=_csr(n=-1)) == ESHAPE and _count(csr=_csr(e=-1)) == ESHAPE and _count(csr=_csr(b=-1)) == ESHAPE
    assert _count(cap=-1) == ESHAPE and _count(cap=65537) == ESHAPE and _count(cap=0) == ESHAPE
    assert _count(csr=_csr(n=40000), cap=65536) == ESHAPE and "int32" in err()   # n_nodes * max_nodes_per_graph > INT32_MAX
    need = lib.gnf_adj_report_workspace_bytes(3, 40, 20)
    assert _count(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _count(cap=65536, ws_bytes=need) == EWORKSPACE                        # the bound itself is accepted
    assert _count(thr=0.0, ws_bytes=need - 1) == EWORKSPACE and _count(ld=9, ws_bytes=need - 1) == EWORKSPACE
    # ---- fill
    assert _fill(dist=False) == EINVAL
    for name in ("z", "rowptr", "senders", "receivers", "cls", "score", "ws"):
        assert _fill(**{name: None}) == EINVAL, name
    assert _fill(d=0) == ESHAPE and _fill(ld=7) == ESHAPE and _fill(b=-1) == ESHAPE and _fill(n=-1) == ESHAPE
    assert _fill(cap=-1) == ESHAPE and _fill(cap=0) == ESHAPE and _fill(cap=65537) == ESHAPE and _fill(ecap=-1) == ESHAPE
    assert _fill(n=40000, cap=65536) == ESHAPE
    assert _fill(ws_bytes=need - 1) == EWORKSPACE
    assert _fill(ecap=0, senders=None, receivers=None, cls=None, score=None, ws_bytes=need - 1) == EWORKSPACE
    assert _fill(ecap=0, senders=None, receivers=None, cls=None, score=None, ws_bytes=need) == 0   # nothing to write: no launch
    # ---- select
    for name in ("score", "cls", "rowptr", "seg", "stat", "count"):
        assert _select(**{name: None}) == EINVAL, name
    assert _select(q=None, nq=1) == EINVAL
    assert _select(n_seg=-1) == ESHAPE and _select(n_seg=1 << 31) == ESHAPE and _select(n=-1) == ESHAPE
    assert _select(ecap=-1) == ESHAPE and _select(q=(0.5,) * 17) == ESHAPE and _select(nq=-1) == ESHAPE
    for bad in (-0.01, 1.01, float("nan")):
        assert _select(q=(0.5, bad)) == ESHAPE and "q[1]" in err()
    assert _select(n_seg=0) == 0 and _select(n_seg=0, q=(0.0, 1.0), score=None, cls=None, ecap=0) == 0   # no segment: no launch
    assert _select(n_seg=0, stat=None, count=None) == 0              # ... and its outputs are empty arrays


def test_python_layer_argument_errors():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd import adj_loss, encoder
    assert gnf_amd.reconstruction_report is adj_loss.reconstruction_report
    assert gnf_amd.predicted_graph is adj_loss.predicted_graph and gnf_amd.error_graph is adj_loss.error_graph
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    for kw in ({}, {"max_nodes_per_graph": 3}, {"per_graph": True}, {"distance_fn": adj_loss.sigmoid_l2(3.0, 2.0)},
               {"distance_fn": adj_loss.hacky_sigmoid_l2}, {"edge_capacity": 10, "n_node_host": [3]}):
        with pytest.raises(_abi.GnfError):                           # CPU tensors: no fallback
            adj_loss.reconstruction_report(g, g, **kw)
    with pytest.raises(NotImplementedError):
        adj_loss.reconstruction_report(g, g, distance_fn=lambda nodes: nodes)
    with pytest.raises(NotImplementedError):
        adj_loss.reconstruction_report(g, g, distance_fn=adj_loss.sigmoid_l2)
    other = graph_from_arrays([4], [0], [], [], np.zeros((4, 4), np.float32))
    for kw in ({"quantiles": (0.5, 1.5)}, {"quantiles": (-0.1,)}, {"quantiles": (0.5,) * 17}, {"edge_capacity": -1}):
        with pytest.raises(ValueError):
            adj_loss.reconstruction_report(g, g, **kw)
    with pytest.raises(ValueError):
        adj_loss.reconstruction_report(other, g)                     # node totals differ
    with pytest.raises(ValueError):
        adj_loss.error_graph({}, 4)
    with pytest.raises(ValueError):
        adj_loss.error_graph({}, "missing")
    assert adj_loss.REPORT_CLASSES == {"correct": 1, "false_positive": 2, "false_negative": 3}
    import inspect
    sig = inspect.signature(adj_loss.reconstruction_report)
    assert list(sig.parameters) == ["gnn_output", "graph_phs", "distance_fn", "threshold", "quantiles", "per_graph",
                                    "edge_capacity", "max_nodes_per_graph", "n_node_host"]
    assert sig.parameters["threshold"].default == 0.5 and sig.parameters["quantiles"].default == (0, .25, .5, .75, 1)
    assert inspect.signature(encoder.evaluate).parameters["report"].default is False
