"""gnf_amd.adj_loss.reconstruction_report (gnf_adj_report_count_f32 / gnf_adj_report_fill / gnf_score_select_f32) on the MI355X.

Inputs: adj_report_ref.BATCHES - graphs of [1, 0, 17, 16, 33, 65, 2, 64] nodes, embeddings with duplicate rows (equal scores), a
directed true graph with duplicate edges and self loops (one batch symmetric), D in {1, 7, 64, 1025}; 1025 is the width at
which the count kernel's 16-row tile leaves LDS (it keeps no column tile at any width).  test_adj_report_cpu.py asserts the
margin condition and the class counts on every one of them.

Everything here is an equality.  Integers (classes, order, rowptr, counts) against the float64 twin on margin-ok batches at
threshold 0.5; scores bit for bit against flow.pred_adj; the predicted sub-list bit for bit against flow.decode_graphs at any
threshold (the same arithmetic: no margin needed); order statistics bit for bit against the twin's selection on the device's own
scores; the interpolated quantiles against the twin's two-operation float64 form of the same statistics."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adj_loss_ref as R
import adj_report_ref as A
from helpers import SENTINEL_BITS, GuardBanded, graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("cls", "score", "class_pairs", "totals", "fp_quantiles", "fn_quantiles", "fp_count", "fn_count")
N = sum(R.SIZES)
OFF = np.concatenate([[0], np.cumsum(R.SIZES)]).astype(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _token(dist):
    from gnf_amd import adj_loss
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    if dist == R.SCALED_HACKY:
        return scaled_hacky_sigmoid_l2
    return adj_loss.hacky_sigmoid_l2 if dist == R.HACKY else adj_loss.sigmoid_l2(dist[0], dist[1])


def _graphs(z, graph):
    """(embeddings GraphsTuple without edges, true GraphsTuple) on the device"""
    n_edge, s, r = graph
    none = np.zeros(0, np.int32)
    emb = graph_from_arrays(R.SIZES, np.zeros(len(R.SIZES), np.int32), none, none, z, DEV)
    true = graph_from_arrays(R.SIZES, n_edge, s, r, np.zeros((len(z), 1), np.float32), DEV)
    return emb, true


@functools.lru_cache(maxsize=None)
def _case(i):
    """batch i of A.BATCHES: (emb, true, token, twin report, device report batch-wide, device report per graph) - once"""
    from gnf_amd.adj_loss import reconstruction_report
    d, dist, sym, gs = A.BATCHES[i]
    seed, z, graph = A.batch(d, dist, sym, gs)
    assert seed is not None
    emb, true = _graphs(z, graph)
    tok = _token(dist)
    ref = A.report(z, R.SIZES, graph[1], graph[2], dist)
    return emb, true, tok, ref, reconstruction_report(emb, true, tok), reconstruction_report(emb, true, tok, per_graph=True)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous().view(torch.int32))


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(_np(a.reshape(-1).contiguous().view(torch.uint8)), _np(b.reshape(-1).contiguous().view(torch.uint8)))


IDS = [f"D{d}-{dist[0]:g}-{dist[1]:g}-{'scaled' if dist[2] else 'raw'}{'-sym' if sym else ''}" for d, dist, sym, _ in A.BATCHES]


# ---- 1. the edge list against the float64 twin -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(A.BATCHES)), ids=IDS)
def test_edge_list_classes_and_counts_equal_the_twin(i):
    from gnf_amd import adj_loss
    emb, true, tok, ref, rep, per = _case(i)
    g = rep["graph"]
    assert g.nodes is emb.nodes and g.n_node is true.n_node and g.senders.dtype == g.receivers.dtype == torch.int32
    assert rep["cls"].dtype == torch.int32 and rep["score"].dtype == torch.float32 and g.edges.dtype == torch.float32
    assert rep["class_pairs"].dtype == rep["totals"].dtype == torch.int64 and rep["class_pairs"].shape == (len(R.SIZES), 3)
    assert all(v.device.type == "cuda" for k, v in rep.items() if k not in ("graph", "csr"))
    for name, got in (("senders", g.senders), ("receivers", g.receivers), ("cls", rep["cls"]), ("n_edge", g.n_edge),
                      ("rowptr", rep["csr"].rowptr), ("class_pairs", rep["class_pairs"]), ("totals", rep["totals"])):
        np.testing.assert_array_equal(_np(got), ref[name], err_msg=name)
    np.testing.assert_array_equal(_np(g.edges), ref["cls"].astype(np.float32))    # complete_mat's weights
    assert rep["csr"].col is g.senders and rep["csr"].n_edges == int(ref["totals"][0]) == len(ref["cls"])
    # cls in {1, 3}: the true batch's deduplicated, loop-free, in-graph edges, in order
    ts, tr = A.true_edges(R.SIZES, _np(true.senders), _np(true.receivers))
    keep = np.isin(_np(rep["cls"]), (1, 3))
    np.testing.assert_array_equal(_np(g.senders)[keep], ts)
    np.testing.assert_array_equal(_np(g.receivers)[keep], tr)
    # class_pairs[:, 1:] are binary_loss' ordered-pair counts
    loss = adj_loss.binary_loss(emb, true, tok)
    assert torch.equal(rep["class_pairs"][:, 1], loss["false_positive_pairs"])
    assert torch.equal(rep["class_pairs"][:, 2], loss["false_negative_pairs"])
    # the per-graph call differs in the quantile entries only
    for k in ("cls", "score", "class_pairs", "totals"):
        assert torch.equal(per[k], rep[k]), k
    assert torch.equal(per["graph"].senders, g.senders) and torch.equal(per["csr"].rowptr, rep["csr"].rowptr)


# ---- 2. scores: the bits of pred_adj ---------------------------------------------------------------------------------------
def _pred_adj_scores(emb, tok, senders, receivers):
    """pred_adj(...)[g][r, s] of every listed pair, as int32 bit patterns"""
    from gnf_amd.flow import pred_adj
    blocks = pred_adj(emb, tok)
    gid = np.repeat(np.arange(len(R.SIZES)), R.SIZES)
    out = np.empty(len(senders), np.int32)
    for g, blk in enumerate(blocks):
        m = gid[receivers] == g
        b = _bits(blk).reshape(R.SIZES[g], R.SIZES[g])
        out[m] = b[receivers[m] - OFF[g], senders[m] - OFF[g]]
    return out


@pytest.mark.parametrize("i", range(len(A.BATCHES)), ids=IDS)
def test_scores_have_the_bits_of_pred_adj(i):
    emb, true, tok, ref, rep, _ = _case(i)
    s, r = _np(rep["graph"].senders), _np(rep["graph"].receivers)
    want = _pred_adj_scores(emb, tok, s, r)
    np.testing.assert_array_equal(_bits(rep["score"]), want)
    sc, cl = _np(rep["score"]), _np(rep["cls"])
    assert (sc[cl != 3] > 0.5).all() and (sc[cl == 3] <= 0.5).all() and len(np.unique(sc)) < len(sc)


def test_tuned_sigmoid_parameters_are_read_at_run_time():
    from gnf_amd.adj_loss import TunedSigmoidL2, reconstruction_report, sigmoid_l2
    emb, true, _, _, _, _ = _case(1)
    tok = TunedSigmoidL2(10.0, 1.0)
    first = reconstruction_report(emb, true, tok)
    fixed = reconstruction_report(emb, true, sigmoid_l2(10.0, 1.0))
    for k in KEYS:
        assert _same_bytes(first[k], fixed[k]), k
    tok.params.copy_(torch.tensor([3.0, 2.0], device=DEV))   # an optimiser step on the device
    second = reconstruction_report(emb, true, tok)
    fixed = reconstruction_report(emb, true, sigmoid_l2(3.0, 2.0))
    assert not torch.equal(second["totals"], first["totals"])
    for k in ("cls", "score", "class_pairs", "totals", "fp_count", "fn_count"):
        assert torch.equal(second[k], fixed[k]), k
    s, r = _np(second["graph"].senders), _np(second["graph"].receivers)
    np.testing.assert_array_equal(_bits(second["score"]), _pred_adj_scores(emb, tok, s, r))


# ---- 3. the predicted sub-list is decode_graphs' edge list -----------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.3, 0.5, 0.9])
@pytest.mark.parametrize("i", [1, 3, 6], ids=[IDS[1], IDS[3], IDS[6]])
def test_predicted_sub_list_equals_decode_graphs(i, threshold):
    from gnf_amd.adj_loss import error_graph, predicted_graph, reconstruction_report
    from gnf_amd.flow import decode_graphs
    emb, true, tok, _, at_half, _ = _case(i)
    rep = at_half if threshold == 0.5 else reconstruction_report(emb, true, tok, threshold=threshold)
    dec = decode_graphs(emb, threshold=threshold, self_loops=False, distance_fn=tok)
    pred = predicted_graph(rep)
    assert int(dec["total_edges"]) == int(rep["totals"][1] + rep["totals"][2]) > 0
    assert torch.equal(pred["graph"].senders, dec["graph"].senders) and torch.equal(pred["graph"].receivers, dec["graph"].receivers)
    assert torch.equal(pred["graph"].n_edge, dec["graph"].n_edge)
    assert set(_np(pred["cls"]).tolist()) == {1, 2} and bool((pred["score"] > threshold).all())
    # the single classes partition the list
    parts = [error_graph(rep, c) for c in ("correct", "false_positive", "false_negative")]
    assert [int(p["cls"].shape[0]) for p in parts] == _np(rep["totals"][1:]).tolist()
    for c, p in zip((1, 2, 3), parts):
        assert bool((p["cls"] == c).all()) and torch.equal(p["graph"].n_edge, rep["class_pairs"][:, c - 1].to(torch.int32))
        assert torch.equal(p["graph"].edges, p["cls"].to(torch.float32))
    fn = parts[2]
    if fn["score"].numel():
        assert bool((fn["score"] <= threshold).all())


# ---- 4. order statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(A.BATCHES)), ids=IDS)
def test_quantiles_equal_the_twins_selection_on_the_devices_scores(i):
    from gnf_amd.adj_loss import score_quantiles
    from gnf_amd.graphs import node_offsets_of
    emb, true, tok, ref, rep, per = _case(i)
    score, cls, rowptr = _np(rep["score"]), _np(rep["cls"]), _np(rep["csr"].rowptr)
    for report, seg in ((rep, np.asarray([0, N])), (per, OFF)):
        stat, count = A.segment_stats(score, cls, rowptr, seg, A.QUANTILES)
        dev_seg = torch.as_tensor(seg.astype(np.int32)).to(DEV)
        sel = score_quantiles(rep["score"], rep["cls"], rep["csr"].rowptr, dev_seg, A.QUANTILES)
        np.testing.assert_array_equal(_bits(sel["stat"]), stat.view(np.int32))        # bit for bit, NaN of empty classes too
        np.testing.assert_array_equal(_np(sel["count"]), count)
        want = np.stack([[A.interpolate(stat[s, c], count[s, c], A.QUANTILES) for c in (0, 1)] for s in range(len(seg) - 1)])
        np.testing.assert_array_equal(_np(sel["quantiles"]), want)                    # the same two float64 operations
        squeeze = (lambda a: a[0]) if len(seg) == 2 else (lambda a: a)
        for c, name in ((0, "fp"), (1, "fn")):
            assert report[name + "_quantiles"].dtype == torch.float64 and report[name + "_count"].dtype == torch.int64
            np.testing.assert_array_equal(_np(report[name + "_quantiles"]), squeeze(want[:, c]))
            np.testing.assert_array_equal(_np(report[name + "_count"]), squeeze(count[:, c]))
    assert per["fp_quantiles"].shape == (len(R.SIZES), len(A.QUANTILES)) and rep["fp_quantiles"].shape == (len(A.QUANTILES),)
    assert torch.equal(per["fp_count"], rep["class_pairs"][:, 1]) and int(rep["fn_count"]) == int(rep["totals"][3])
    assert bool(torch.isnan(per["fp_quantiles"][:2]).all()) and int(per["fp_count"].max()) > 256 < int(per["fn_count"].max())
    assert torch.equal(torch.as_tensor(OFF).to(DEV), node_offsets_of(true))
    # against numpy's own quantile on the same scores: the bound test_adj_report_cpu.py derives
    for c, name in ((2, "fp"), (3, "fn")):
        x = score[cls == c].astype(np.float64)
        assert np.abs(_np(rep[name + "_quantiles"]) - np.quantile(x, A.QUANTILES)).max() <= 8.0 * 2.0 ** -53 * x.max()


def _raw_select(score, cls, rowptr, seg, quantiles, n_nodes=None, capacity=None):
    """gnf_score_select_f32 on host arrays: (stat float32 [S, 2, nq, 2], count int64 [S, 2])"""
    from gnf_amd import _abi
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(DEV)
    sc, cl, rp, sg = dev(score, np.float32), dev(cls, np.int32), dev(rowptr, np.int32), dev(seg, np.int32)
    n_seg, nq = len(seg) - 1, len(quantiles)
    stat = torch.full((n_seg, 2, nq, 2), -7.0, dtype=torch.float32, device=DEV)
    count = torch.full((n_seg, 2), -7, dtype=torch.int64, device=DEV)
    rc = _abi.lib().gnf_score_select_f32(_abi.ptr(sc), _abi.ptr(cl), _abi.ptr(rp), _abi.ptr(sg), n_seg,
                                         len(rowptr) - 1 if n_nodes is None else n_nodes,
                                         len(score) if capacity is None else capacity, (C.c_double * max(nq, 1))(*quantiles), nq,
                                         _abi.ptr(stat), _abi.ptr(count), _abi.stream_ptr(torch.device(DEV)))
    _abi.check(rc, "gnf_score_select_f32")
    torch.cuda.synchronize()
    return _np(stat), _np(count)


def _check_select(score, cls, rowptr, seg, quantiles=(0.0, 0.25, 0.5, 0.75, 1.0)):
    score = np.ascontiguousarray(score, np.float32)
    stat, count = _raw_select(score, cls, rowptr, seg, quantiles)
    want, n = A.segment_stats(score, np.asarray(cls), rowptr, seg, quantiles)
    np.testing.assert_array_equal(stat.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(count, n)
    return stat, count


def test_select_on_hand_made_arrays():
    """one node per segment: rowptr are the segments' entry offsets"""
    rng = np.random.default_rng(3)
    f32 = lambda bits: np.asarray(bits, np.uint32).view(np.float32)
    # n = 0, 1, 2 and a segment holding no entry of either class, side by side
    sizes = [0, 1, 2, 5]
    score = rng.random(8).astype(np.float32)
    cls = np.array([2, 3, 3, 1, 1, 1, 1, 1])
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    stat, count = _check_select(score, cls, rowptr, np.arange(5))
    assert count.tolist() == [[0, 0], [1, 0], [0, 2], [0, 0]] and np.isnan(stat[0]).all() and np.isnan(stat[3]).all()
    assert (stat[1, 0] == score[0]).all() and np.isnan(stat[1, 1]).all()
    assert stat[2, 1, 0].tolist() == [score[1:3].min(), score[1:3].max()] and (stat[2, 1, -1] == score[1:3].max()).all()
    # all scores equal; scores that differ in the lowest byte only, and in the highest only
    for bits in (np.full(300, 0x3F000000), 0x3F000000 + rng.integers(0, 256, 300), (rng.integers(0, 0x7F, 300) << 24) + 0x123456):
        x = f32(bits)
        stat, _ = _check_select(x, np.full(300, 2), [0, 300], [0, 1])
        assert stat[0, 0, 0, 0] == x.min() and stat[0, 0, -1, 1] == x.max()        # q = 0 and q = 1
    # 257 and 65 537 entries of a class, the other class interleaved, ties; every q
    for n in (257, 65537):
        x = rng.random(2 * n).astype(np.float32)
        x[::7] = x[0]
        cls = np.tile([2, 3], n)
        _check_select(x, cls, [0, 2 * n], [0, 1], (0.0, 0.001, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.999, 1.0))
    # a NaN score sorts last: only the top statistic sees it
    x = np.array([0.5, np.nan, 0.25, 0.125], np.float32)
    stat, count = _check_select(x, [3, 3, 3, 3], [0, 4], [0, 1], (0.0, 0.5, 1.0))
    assert count[0].tolist() == [0, 4] and stat[0, 1, 0].tolist() == [0.125, 0.25] and np.isnan(stat[0, 1, 2]).all()
    # no quantile: counts only; a capacity below the list's end cuts the segments, offsets past the arrays are clamped
    stat, count = _raw_select(x, [3, 3, 3, 3], [0, 4], [0, 1], ())
    assert count[0].tolist() == [0, 4]
    stat, count = _raw_select(x, [3, 3, 3, 3], [0, 400], [0, 7], (0.0, 1.0), n_nodes=1, capacity=3)
    assert count[0].tolist() == [0, 3] and np.isnan(stat[0, 1, 1]).all() and stat[0, 1, 0, 0] == 0.25


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    from gnf_amd.adj_loss import reconstruction_report
    emb, true, tok, _, rep, per = _case(2)
    for first, kw in ((rep, {}), (per, {"per_graph": True})):
        again = reconstruction_report(emb, true, tok, **kw)
        for k in KEYS:
            assert _same_bytes(first[k], again[k]), k
        for k in ("senders", "receivers", "n_edge", "edges"):
            assert torch.equal(getattr(first["graph"], k), getattr(again["graph"], k)), k
        assert torch.equal(first["csr"].rowptr, again["csr"].rowptr)


# ---- 6. row stride, guard bands, capacity ----------------------------------------------------------------------------------
def _raw_report(zwin, ld, d, true, cap, capacity, guard=64):
    """count + fill through the raw entry points into sentinel-filled buffers; the outputs sit `guard` elements inside"""
    from gnf_amd import _abi
    from gnf_amd.adj_loss import distance_desc
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    from gnf_amd.graphs import csr_desc, csr_of
    lib, dev = _abi.lib(), torch.device(DEV)
    b = len(R.SIZES)
    desc = csr_desc(true, csr_of(true), node_offsets=True)
    dist = distance_desc(scaled_hacky_sigmoid_l2, dev)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=DEV)
    n_edge = torch.empty(b, dtype=torch.int32, device=DEV)
    pairs = torch.empty((b, 3), dtype=torch.int64, device=DEV)
    totals = torch.empty(4, dtype=torch.int64, device=DEV)
    ws_bytes = lib.gnf_adj_report_workspace_bytes(b, N, cap)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _abi.check(lib.gnf_adj_report_count_f32(C.byref(desc), C.byref(dist), C.c_void_p(zwin.data_ptr()), ld, d, cap, 0.5,
                                            _abi.ptr(rowptr), _abi.ptr(n_edge), _abi.ptr(pairs), _abi.ptr(totals), _abi.ptr(ws),
                                            ws_bytes, _abi.stream_ptr(dev)), "count")
    bufs = {k: torch.full((capacity + 2 * guard,), SENTINEL_BITS, dtype=torch.int32, device=DEV)
            for k in ("senders", "receivers", "cls", "score")}
    at = {k: C.c_void_p(v.data_ptr() + 4 * guard) for k, v in bufs.items()}
    _abi.check(lib.gnf_adj_report_fill(C.byref(dist), C.c_void_p(zwin.data_ptr()), ld, d, b, N, cap, _abi.ptr(rowptr), capacity,
                                       at["senders"], at["receivers"], at["cls"], at["score"], _abi.ptr(ws), ws_bytes,
                                       _abi.stream_ptr(dev)), "fill")
    torch.cuda.synchronize()
    return rowptr, n_edge, pairs, totals, bufs


@pytest.mark.parametrize("d,ld,c0", [(7, 13, 3), (64, 72, 4)])
def test_row_stride_guard_bands_and_a_short_capacity(d, ld, c0):
    i = 1 if d == 7 else 2
    emb, true, tok, ref, rep, _ = _case(i)
    from gnf_amd.adj_loss import reconstruction_report
    gb = GuardBanded(N, d, ld, c0=c0, device=DEV, fill=_np(emb.nodes))
    assert gb.window.stride(0) == ld and gb.window.data_ptr() != gb.bits.data_ptr()
    strided = reconstruction_report(emb.replace(nodes=gb.window), true, tok, per_graph=True, max_nodes_per_graph=70)
    for k in ("cls", "score", "class_pairs", "totals"):
        assert torch.equal(strided[k], rep[k]), k
    gb.check_guard()
    total, guard = int(ref["totals"][0]), 64
    for capacity in (total, total - 1000, 0):
        rowptr, n_edge, pairs, totals, bufs = _raw_report(gb.window, ld, d, true, 65, capacity, guard)
        assert torch.equal(totals, rep["totals"]) and torch.equal(pairs, rep["class_pairs"])   # the full counts either way
        assert torch.equal(rowptr, rep["csr"].rowptr) and torch.equal(n_edge, rep["graph"].n_edge)
        want = {"senders": rep["graph"].senders, "receivers": rep["graph"].receivers, "cls": rep["cls"],
                "score": rep["score"].view(torch.int32)}
        for k, buf in bufs.items():
            assert torch.equal(buf[guard:guard + capacity], want[k][:capacity]), k
            assert bool((buf[:guard] == SENTINEL_BITS).all()) and bool((buf[guard + capacity:] == SENTINEL_BITS).all()), k
    gb.check_guard()
    # the Python layer with a capacity below the total: the valid prefix, the full totals, quantiles of the valid entries
    short = reconstruction_report(emb, true, tok, edge_capacity=total - 1000, n_node_host=R.SIZES)
    assert short["cls"].shape == (total - 1000,) and torch.equal(short["totals"], rep["totals"])
    assert torch.equal(short["cls"], rep["cls"][:total - 1000]) and torch.equal(short["score"], rep["score"][:total - 1000])
    stat, count = A.segment_stats(_np(short["score"]), _np(short["cls"]), np.minimum(_np(rep["csr"].rowptr), total - 1000),
                                  [0, N], A.QUANTILES)
    assert int(short["fp_count"]) == count[0, 0] and int(short["fn_count"]) == count[0, 1]
    np.testing.assert_array_equal(_np(short["fp_quantiles"]), A.interpolate(stat[0, 0], count[0, 0], A.QUANTILES))


def test_empty_batches_give_zeroed_outputs():
    from gnf_amd.adj_loss import predicted_graph, reconstruction_report
    none = np.zeros(0, np.int32)
    for sizes in ([], [0, 0], [1, 0, 1]):
        n = sum(sizes)
        g = graph_from_arrays(sizes, np.zeros(len(sizes), np.int32), none, none, np.zeros((n, 3), np.float32), DEV)
        rep = reconstruction_report(g, g, per_graph=True)
        assert rep["totals"].tolist() == [0, 0, 0, 0] and rep["cls"].shape == (0,) and rep["score"].shape == (0,)
        assert rep["class_pairs"].shape == (len(sizes), 3) and not bool(rep["class_pairs"].any())
        assert rep["csr"].rowptr.tolist() == [0] * (n + 1) and rep["graph"].n_edge.tolist() == [0] * len(sizes)
        assert rep["fp_quantiles"].shape == (len(sizes), 5) and bool(torch.isnan(rep["fp_quantiles"]).all())
        assert rep["fn_count"].tolist() == [0] * len(sizes)
        assert predicted_graph(rep)["graph"].senders.shape == (0,)


# ---- 7. capture ------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_new_embeddings():
    """With edge_capacity and n_node_host nothing is read back and nothing synchronises: the call is captured on one stream, z
    is overwritten in place, and the replay equals an eager call on the new z bit for bit."""
    from gnf_amd.adj_loss import reconstruction_report
    emb, true, tok, ref, _, _ = _case(2)
    emb = emb.replace(nodes=emb.nodes.clone())
    capacity = N * 65
    kw = dict(per_graph=True, edge_capacity=capacity, n_node_host=R.SIZES)
    reconstruction_report(emb, true, tok, **kw)                                     # (the first launches: CSR and offsets caches)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = reconstruction_report(emb, true, tok, **kw)
    for seed in (11, 12):
        emb.nodes.copy_(torch.as_tensor(R.embeddings(R.SIZES, 64, seed)).to(DEV))
        for k in KEYS:
            captured[k].zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = reconstruction_report(emb, true, tok, per_graph=True)
        total = int(eager["totals"][0])
        assert 0 < total <= capacity and total != int(ref["totals"][0])
        assert torch.equal(captured["totals"], eager["totals"]) and torch.equal(captured["class_pairs"], eager["class_pairs"])
        assert torch.equal(captured["cls"][:total], eager["cls"]) and torch.equal(captured["score"][:total], eager["score"])
        assert torch.equal(captured["graph"].senders[:total], eager["graph"].senders)
        assert torch.equal(captured["csr"].rowptr, eager["csr"].rowptr)
        for k in ("fp_quantiles", "fn_quantiles", "fp_count", "fn_count"):
            assert _same_bytes(captured[k], eager[k]), k


# ---- 8. encoder.evaluate ---------------------------------------------------------------------------------------------------
@pytest.fixture
def _initialiser_state():
    """the weight initialisers' process-wide generator is left as it was found: tests that run later and draw their weights
    from it see the numbers they saw before this file existed"""
    from gnf_amd import gnn
    state = gnn._GEN.get_state()
    yield
    gnn._GEN.set_state(state)


def test_evaluate_with_report_changes_nothing_else(_initialiser_state):
    from gnf_amd import adj_loss, datasets, encoder, gnn
    gnn.set_random_seed(7)
    hp = dict(node_dim=8, latent=32, K=2, activation="leaky_relu", bias_init_stddev=0.3, num_timesteps=2, weight_sharing=True,
              use_batch_norm=True, use_layer_norm=False, residual=True, test_local_stats=True, agg="mean", combine="agg",
              epsilon=2.0)
    enc = encoder.make_encoder(hp)
    graph = datasets.GraphDataset("graph_rnn_grid_small", 8, 0.3, seed=1).get_random_test_batch(4, torch.device(DEV))
    plain = encoder.evaluate(enc, graph)
    full = encoder.evaluate(enc, graph, report=True)
    assert set(full) == set(plain) | {"report"}

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,))
        elif isinstance(a, torch.Tensor):
            assert _same_bytes(a, b), path
        elif isinstance(a, tuple):   # a GraphsTuple
            for x, y in zip(a, b):
                same(x, y, path)
        else:
            assert a is b or a == b, path
    for k in plain:
        same(plain[k], full[k], (k,))
    rep = full["report"]
    assert torch.equal(rep["class_pairs"][:, 1], full["loss"]["false_positive_pairs"])
    assert torch.equal(rep["class_pairs"][:, 2], full["loss"]["false_negative_pairs"])
    assert float(adj_loss.total_incorrect_edges(full["loss"])) == float(rep["totals"][2] + rep["totals"][3]) / 2.0
    per = encoder.evaluate(enc, graph, report={"per_graph": True, "quantiles": (0.5,)}, max_nodes_per_graph=400)["report"]
    assert per["fp_quantiles"].shape == (4, 1) and torch.equal(per["cls"], rep["cls"])
