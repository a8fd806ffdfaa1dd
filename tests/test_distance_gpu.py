"""One distance function from the loss to the decoded graphs, with parameters that may live on the device (include/gnf_distance.h):
gnf_pred_adj_dist_f32, gnf_adj_edges_count_dist_f32 and gnf_adj_loss_dist_f32 on the MI355X, through flow.pred_adj,
flow.decode_graphs, adj_loss.binary_loss(grad_params=...), adj_loss.TunedSigmoidL2 and train.EncoderTrainer(tune_sigmoid=True).

Inputs: graphs of [1, 0, 17, 16, 33, 65, 2, 64] nodes (adj_loss_ref.SIZES).  The decoder checks are exact (bits, edge sets,
counts) and need no condition on the embeddings; the parameter gradient is compared with the float64 closed form of
tests/distance_ref.py on the first seed whose logits keep 2 delta from the kinks (adj_loss_ref.pick_seed), under
  dtemp   sum [(0.25 delta_ij + 2^-22) |w_ij| + |p_ij - t_ij| delta_ij / |temp|] + 2^-22 |dL/dtemp|
  dshift  |temp| sum (0.25 delta_ij + 2^-22) + 2^-22 |dL/dshift|
(distance_ref.param_grad_bounds; tests/test_distance_cpu.py holds a float32 numpy restatement to the same bound).  With the
unscaled distance at D >= 200 every pair of these embeddings lies beyond the clip: the gradient is exactly zero there, on both
sides.

Worst error / bound measured on an MI355X: parameter gradient 0.0101 over the 30 cases (D = 7, sigmoid_l2(20, 1), hard
labels: dtemp 0.0101, dshift 0.0066), pred_adj's blocks 0.125 (D = 7, sigmoid_l2(20, 1)); no bound was changed afterwards.

The capture test: replay and eager agree bit for bit before the optimiser step (sum_loss 7873.477473) and after it (temp 9.99,
shift 0.99: 3062.501473 both ways).  While gnf_adj_loss_dist_f32 zeroed its workspace with a memset node the second and later
replays lost bitmap bits and row sums (3513.60 to 4046.47 over six processes); it zeroes with a kernel now."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gnf_amd import _abi, adj_loss, encoder, flow
from gnf_amd.flow import scaled_hacky_sigmoid_l2
from gnf_amd.graphs import csr_desc, csr_of
from gnf_amd.train import EncoderTrainer, encoder_trainer_state, load_encoder_trainer_state
from helpers import GuardBanded, graph_from_arrays

import adj_loss_ref as R
import distance_ref as DR
import timestep_gnn_grad_ref as G
import timestep_gnn_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("sum_loss", "mean_loss", "loss_per_graph", "false_positive_pairs", "false_negative_pairs")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _abi.lib()


def _graphs(z, sizes, graph):
    """(embeddings GraphsTuple without edges, true GraphsTuple) on the device"""
    n_edge, s, r = graph
    none = np.zeros(0, np.int32)
    emb = graph_from_arrays(sizes, np.zeros(len(sizes), np.int32), none, none, z, DEV)
    true = graph_from_arrays(sizes, n_edge, s, r, np.zeros((len(z), 1), np.float32), DEV)
    return emb, true


def _fixed(dist):
    """the fixed token of a (temp, shift, scaled) triple"""
    if dist == R.HACKY:
        return adj_loss.hacky_sigmoid_l2
    assert dist[2]
    return adj_loss.sigmoid_l2(dist[0], dist[1])


def _tuned(dist):
    return adj_loss.TunedSigmoidL2(dist[0], dist[1], scale_by_sqrt_dim=dist[2])


def _edges_of_blocks(blocks, sizes, threshold):
    """(senders, receivers) of `block > threshold`, receivers ascending and senders ascending within a receiver"""
    ss, rr, o = [], [], 0
    for blk, ng in zip(blocks, sizes):
        ij = torch.nonzero(blk > threshold)       # row-major: i ascending, j ascending within i
        rr.append(ij[:, 0] + o), ss.append(ij[:, 1] + o)
        o += ng
    return torch.cat(ss).to(torch.int32), torch.cat(rr).to(torch.int32)


# ---- 1. decoder consistency ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder_batch(d):
    z = R.embeddings(R.SIZES, d, 5, duplicate_rows=True)
    return z, R.true_graph(R.SIZES, 5)


DECODER_TOKENS = {"hacky": (R.HACKY, lambda: adj_loss.hacky_sigmoid_l2),
                  "sigmoid_3_2": (R.sigmoid_l2(3.0, 2.0), lambda: adj_loss.sigmoid_l2(3.0, 2.0)),
                  "sigmoid_20_1": (R.sigmoid_l2(20.0, 1.0), lambda: adj_loss.sigmoid_l2(20.0, 1.0)),
                  "tuned_3_2": (R.sigmoid_l2(3.0, 2.0), lambda: adj_loss.TunedSigmoidL2(3.0, 2.0))}


@pytest.mark.parametrize("name", list(DECODER_TOKENS))
@pytest.mark.parametrize("d", [7, 1030])   # the LDS-tile and the global-read route of both decode kernels
def test_loss_pred_adj_and_decode_graphs_agree(d, name):
    dist, make = DECODER_TOKENS[name]
    tok = make()
    z, graph = _decoder_batch(d)
    emb, true = _graphs(z, R.SIZES, graph)
    blocks = flow.pred_adj(emb, distance_fn=tok)
    assert [tuple(b.shape) for b in blocks] == [(ng, ng) for ng in R.SIZES]
    # the edge list is `block > threshold`, exactly
    edges = 0
    for thr in (0.1, 0.5, 0.9):
        dec = flow.decode_graphs(emb, threshold=thr, distance_fn=tok)
        s, r = _edges_of_blocks(blocks, R.SIZES, thr)
        assert torch.equal(dec["graph"].senders, s) and torch.equal(dec["graph"].receivers, r), thr
        assert int(dec["total_edges"]) == s.numel()
        assert dec["graph"].n_edge.tolist() == [int((b > thr).sum()) for b in blocks]
        edges += s.numel()
    # the loss's verdict on every pair is the block's
    out = adj_loss.binary_loss(emb, true, distance_fn=tok)
    labels = R.graph_blocks(z, R.SIZES, graph[1], graph[2], dist)
    fp, fn = [], []
    for p, lab in zip(blocks, labels):
        a = torch.as_tensor(lab["a"].astype(np.float32)).to(DEV)
        fp.append(int((p - a > 0.5).sum()))
        fn.append(int((a - p > 0.5).sum()))
    assert out["false_positive_pairs"].tolist() == fp and out["false_negative_pairs"].tolist() == fn
    assert sum(fn) > 100 and (sum(fp) > 100 and edges > 300 or dist == R.HACKY and d == 1030)   # (unscaled, wide: all far apart)
    # and the blocks are sigmoid(u) of the float64 logit, to what fp32 moves the logit by through the sigmoid's slope
    worst = 0.0
    for p, lab, dl in zip(blocks, labels, R.delta(labels, d, dist)):
        with np.errstate(over="ignore"):
            want = np.where(lab["off"], 1.0 / (1.0 + np.exp(-lab["u"])), 0.0)
        err, bound = np.abs(p.cpu().numpy().astype(np.float64) - want), 0.25 * dl + 2.0 ** -22
        if err.size:
            worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
        assert not np.diag(p.cpu().numpy()).any()
    print(f"D={d} {name}: pred_adj error / bound {worst:.3g}, {edges} edges over three thresholds, fp {sum(fp)} fn {sum(fn)}")
    if isinstance(tok, adj_loss.TunedSigmoidL2):
        assert tok.values() == (3.0, 2.0) and tok.params.device.type == "cuda"
        fixed = adj_loss.sigmoid_l2(3.0, 2.0)            # device-resident parameters change no bit
        for a, b in zip(blocks, flow.pred_adj(emb, distance_fn=fixed)):
            assert torch.equal(a, b)
        ref = adj_loss.binary_loss(emb, true, distance_fn=fixed)
        assert all(torch.equal(out[k], ref[k]) for k in KEYS)


def _raw_pred_adj(emb, sizes):
    lib, z = _abi.lib(), emb.nodes
    b, n = len(sizes), int(z.shape[0])
    out = torch.empty(max(sum(s * s for s in sizes), 1), dtype=torch.float32, device=DEV)
    off = torch.empty(b + 1, dtype=torch.int64, device=DEV)
    ws_bytes = lib.gnf_pred_adj_workspace_bytes(b)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    nn = emb.n_node.to(torch.int32).contiguous()
    _abi.check(lib.gnf_pred_adj_f32(_abi.ptr(z), z.stride(0), z.shape[1], _abi.ptr(nn), b, max(sizes), _abi.ptr(out),
                                    _abi.ptr(off), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(torch.device(DEV))), "gnf_pred_adj_f32")
    return out[:sum(s * s for s in sizes)]


def _raw_edges(emb, sizes, thr):
    lib, z = _abi.lib(), emb.nodes
    b, n, cap = len(sizes), int(z.shape[0]), max(sizes)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    n_edge = torch.empty(b, dtype=torch.int32, device=DEV)
    total = torch.empty(1, dtype=torch.int64, device=DEV)
    ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, cap)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    nn = emb.n_node.to(torch.int32).contiguous()
    st = _abi.stream_ptr(torch.device(DEV))
    _abi.check(lib.gnf_adj_edges_count_f32(_abi.ptr(z), z.stride(0), z.shape[1], _abi.ptr(nn), b, n, cap, thr, 0, _abi.ptr(rowptr),
                                           _abi.ptr(n_edge), _abi.ptr(total), _abi.ptr(ws), ws_bytes, st), "gnf_adj_edges_count_f32")
    e = int(total.item())
    s, r = torch.empty(e, dtype=torch.int32, device=DEV), torch.empty(e, dtype=torch.int32, device=DEV)
    _abi.check(lib.gnf_adj_edges_fill(b, n, cap, _abi.ptr(rowptr), e, _abi.ptr(s), _abi.ptr(r), _abi.ptr(ws), ws_bytes, st),
               "gnf_adj_edges_fill")
    return s, r, n_edge


def _raw_loss(emb, true, sizes):
    lib, z = _abi.lib(), emb.nodes
    b, n, d = len(sizes), int(z.shape[0]), int(z.shape[1])
    desc = csr_desc(true, csr_of(true), node_offsets=True)
    spec = _abi.GnfAdjLossSpec(10.0, 1.0, 1, 0, 0.1, 0.5)
    sums2 = torch.empty(2, dtype=torch.float64, device=DEV)
    loss = torch.empty(b, dtype=torch.float64, device=DEV)
    fp, fn = torch.empty(b, dtype=torch.int64, device=DEV), torch.empty(b, dtype=torch.int64, device=DEV)
    g = torch.empty((n, d), dtype=torch.float32, device=DEV)
    ws_bytes = lib.gnf_adj_loss_workspace_bytes(b, n, max(sizes))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _abi.check(lib.gnf_adj_loss_f32(C.byref(desc), _abi.ptr(z), z.stride(0), d, max(sizes), C.byref(spec), _abi.ptr(loss),
                                    _abi.ptr(sums2), _abi.ptr(fp), _abi.ptr(fn), _abi.ptr(g), d, 1.0, _abi.ptr(ws), ws_bytes,
                                    _abi.stream_ptr(torch.device(DEV))), "gnf_adj_loss_f32")
    return {"sum_loss": sums2[0], "mean_loss": sums2[1], "loss_per_graph": loss, "false_positive_pairs": fp,
            "false_negative_pairs": fn, "grad_nodes": g}


@pytest.mark.parametrize("d", [7, 1030])
def test_tuned_10_1_and_the_default_token_give_the_old_entry_points_bits(d):
    z, graph = _decoder_batch(d)
    emb, true = _graphs(z, R.SIZES, graph)
    tuned = adj_loss.TunedSigmoidL2(10.0, 1.0)
    raw = _raw_pred_adj(emb, R.SIZES)
    for tok in (scaled_hacky_sigmoid_l2, tuned, adj_loss.sigmoid_l2(10.0, 1.0)):
        blocks = flow.pred_adj(emb, distance_fn=tok)
        assert torch.equal(torch.cat([b.reshape(-1) for b in blocks]), raw), tok
    assert float(raw.max()) > 0.99 and 0.0 < float(raw[raw > 0].min()) < 0.01
    for thr in (0.1, 0.5, 0.9):
        s, r, n_edge = _raw_edges(emb, R.SIZES, thr)
        for tok in (scaled_hacky_sigmoid_l2, tuned):
            dec = flow.decode_graphs(emb, threshold=thr, distance_fn=tok)
            assert torch.equal(dec["graph"].senders, s) and torch.equal(dec["graph"].receivers, r), (thr, tok)
            assert torch.equal(dec["graph"].n_edge, n_edge)
    want = _raw_loss(emb, true, R.SIZES)
    for tok in (scaled_hacky_sigmoid_l2, tuned):
        got = adj_loss.binary_loss(emb, true, distance_fn=tok, grad="sum")
        for k in KEYS + ("grad_nodes",):
            assert torch.equal(got[k], want[k]), (k, tok)
    with_gp = adj_loss.binary_loss(emb, true, distance_fn=tuned, grad="sum", grad_params=True)
    for k in KEYS + ("grad_nodes",):
        assert torch.equal(with_gp[k], want[k]), k
    assert tuned.values() == (10.0, 1.0)


# ---- 2. parameter gradients --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", DR.GRAD_CASES, ids=DR.case_id)
def test_parameter_gradients_against_float64(c):
    d, dist, soft = c
    seed, z, graph = DR.grad_case(*c)
    assert seed is not None, "no seed in range(16) satisfies the margin condition"
    emb, true = _graphs(z, R.SIZES, graph)
    tok = _tuned(dist)
    out = adj_loss.binary_loss(emb, true, tok, soft, grad="sum", grad_params=True)
    assert set(out) == set(KEYS) | {"grad_nodes", "grad_params"}
    gp = out["grad_params"]
    assert gp.dtype == torch.float32 and gp.shape == (2,) and gp.device.type == "cuda"
    ref = DR.param_grads(z, R.SIZES, graph[1], graph[2], dist, soft)
    bound = DR.param_grad_bounds(z, R.SIZES, graph[1], graph[2], dist, soft)
    got = [float(v) for v in gp.cpu().numpy().astype(np.float64)]
    err = [abs(g - w) for g, w in zip(got, ref)]
    ratio = [e / b if b > 0 else (0.0 if e == 0 else float("inf")) for e, b in zip(err, bound)]
    print(f"[distance] {DR.case_id(c)}: dtemp {got[0]:.9g} ref {ref[0]:.9g} err/bound {ratio[0]:.3g} | dshift {got[1]:.9g} "
          f"ref {ref[1]:.9g} err/bound {ratio[1]:.3g}")
    assert err[0] <= bound[0] and err[1] <= bound[1]
    # the extra sums disturb nothing: every other output has the bits of the fixed token's call (gnf_adj_loss_f32)
    fixed = adj_loss.binary_loss(emb, true, _fixed(dist), soft, grad="sum")
    for k in KEYS + ("grad_nodes",):
        assert torch.equal(out[k], fixed[k]), k
    # grad="mean" scales the parameter gradient as it scales the node gradient; without grad it is the sum's
    n = len(z)
    mean = adj_loss.binary_loss(emb, true, tok, soft, grad="mean", grad_params=True)["grad_params"].cpu().numpy()
    for m, w, b in zip(mean, ref, bound):
        assert abs(float(m) - w / (n * n - n)) <= b / (n * n - n) + 2.0 ** -23 * abs(w) / (n * n - n)
    assert torch.equal(adj_loss.binary_loss(emb, true, tok, soft, grad_params=True)["grad_params"], gp)


# ---- 3. determinism and strides ------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_padded_offset_view_the_contiguous_ones():
    d, ld, c0 = 7, 13, 3
    dist = R.sigmoid_l2(3.0, 2.0)
    seed, z, graph = DR.grad_case(d, dist, True)
    emb, true = _graphs(z, R.SIZES, graph)
    tok = _tuned(dist)
    keys = KEYS + ("grad_nodes", "grad_params")
    a = adj_loss.binary_loss(emb, true, tok, True, grad="sum", grad_params=True)
    b = adj_loss.binary_loss(emb, true, tok, True, grad="sum", grad_params=True)
    assert all(torch.equal(a[k], b[k]) for k in keys) and float(a["grad_params"].abs().min()) > 1.0
    band = GuardBanded(len(z), d, ld, c0=c0, device=DEV, fill=z)
    view = emb.replace(nodes=band.window)
    assert band.window.stride(0) == ld and band.window.data_ptr() % 16 != 0
    c = adj_loss.binary_loss(view, true, tok, True, grad="sum", grad_params=True)
    assert all(torch.equal(a[k], c[k]) for k in keys)
    for thr in (0.1, 0.5):
        x, y = flow.decode_graphs(emb, threshold=thr, distance_fn=tok), flow.decode_graphs(view, threshold=thr, distance_fn=tok)
        assert torch.equal(x["graph"].senders, y["graph"].senders) and torch.equal(x["graph"].receivers, y["graph"].receivers)
    for p, q in zip(flow.pred_adj(emb, distance_fn=tok), flow.pred_adj(view, distance_fn=tok)):
        assert torch.equal(p, q)
    band.check_guard()


def test_an_empty_batch_zeroes_grad_params():
    none = np.zeros(0, np.int32)
    emb = graph_from_arrays([0, 0], [0, 0], none, none, np.zeros((0, 7), np.float32), DEV)
    gp = torch.full((2,), 7.0, device=DEV)
    out = adj_loss.binary_loss(emb, emb, adj_loss.TunedSigmoidL2(3.0, 2.0), grad="sum", grad_params=gp, max_nodes_per_graph=4)
    assert out["grad_params"] is gp and gp.tolist() == [0.0, 0.0]
    assert float(out["sum_loss"]) == 0.0 and out["loss_per_graph"].tolist() == [0.0, 0.0] and out["grad_nodes"].shape == (0, 7)


# ---- 4. device-resident parameters under capture, the trainer ------------------------------------------------------------------
def _graph(batch, x):
    nn, ne, s, r = batch
    return graph_from_arrays(nn, ne, s, r, x, DEV)


def _encoder(c, params=None):
    return encoder.make_encoder(G.family_hp(c)).set_params(G.make_params(c) if params is None else params)


def _e2e_graph():
    seed, x, _, _ = G.pick_e2e("hard")    # no pair of the encoder's output sits at the clip
    assert seed is not None
    return _graph(TR.ring_chord_batch(TR.SIZES), x)


def test_a_captured_loss_and_grads_follows_the_parameters_on_the_device():
    graph = _e2e_graph()
    tr = EncoderTrainer(_encoder(G.E2E_CASE, G.e2e_params()), lr=1e-2, num_train_iters=4, max_nodes_per_graph=64,
                        distance_fn=adj_loss.TunedSigmoidL2(10.0, 1.0), tune_sigmoid=True)
    eager = tr.loss_and_grads(graph)                         # variables, CSRs and the allocator's blocks exist
    torch.cuda.synchronize()
    want0 = (eager["sum_loss"].clone(), tr.grad.clone())
    assert tr.distance_fn.params.data_ptr() == tr.theta[-2:].data_ptr() and tr.distance_fn.values() == (10.0, 1.0)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        res_c = tr.loss_and_grads(graph)
    tr.grad.zero_()
    cg.replay()
    torch.cuda.synchronize()
    first = (res_c["sum_loss"].clone(), tr.grad.clone())
    assert torch.equal(first[0], want0[0]) and torch.equal(first[1], want0[1])
    assert float(tr.grad[-2].abs()) > 0.0 and float(tr.grad[-1].abs()) > 0.0
    tr.apply_gradients()                                     # one Adam launch moves temp and shift with everything else
    torch.cuda.synchronize()
    temp, shift = tr.distance_fn.values()
    assert temp != 10.0 and shift != 1.0
    tr.grad.zero_()
    cg.replay()
    torch.cuda.synchronize()
    second = (res_c["sum_loss"].clone(), tr.grad.clone())
    fresh = tr.loss_and_grads(graph)                         # eager, with the updated temp and shift
    torch.cuda.synchronize()
    print(f"[distance] capture: sum_loss eager {float(want0[0]):.6f}, replay {float(first[0]):.6f}; after the step (temp {temp!r}, "
          f"shift {shift!r}) replay {float(second[0]):.6f}, eager {float(fresh['sum_loss']):.6f}")
    assert torch.equal(second[0], fresh["sum_loss"]) and torch.equal(second[1], tr.grad)
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[1][-2:], first[1][-2:])
    # a trainer that holds the same encoder values but the OLD temp and shift as constants does not reproduce the replay:
    # the replay's numbers come from the device values, not from anything baked in at capture time
    old = adj_loss.binary_loss(fresh["gnn_output"], graph, adj_loss.sigmoid_l2(10.0, 1.0), max_nodes_per_graph=64)
    new = adj_loss.binary_loss(fresh["gnn_output"], graph, adj_loss.sigmoid_l2(temp, shift), max_nodes_per_graph=64)
    assert torch.equal(new["sum_loss"], second[0]) and not torch.equal(old["sum_loss"], second[0])


def test_the_trainer_trains_temp_and_shift_with_one_adam_launch():
    from oracle.gnf_oracle import adam_step
    graph = _e2e_graph()
    plain = EncoderTrainer(_encoder(G.E2E_CASE, G.e2e_params()), lr=1e-2, num_train_iters=20)
    plain.loss_and_grads(graph)
    tr = EncoderTrainer(_encoder(G.E2E_CASE, G.e2e_params()), lr=1e-2, num_train_iters=20,
                        distance_fn=adj_loss.sigmoid_l2(3.0, 2.0), tune_sigmoid=True)
    res = tr.loss_and_grads(graph)
    assert tr.theta.numel() == plain.theta.numel() + 2 == tr.grad.numel() == tr.m.numel() == tr.v.numel()
    assert tr.theta[-2:].tolist() == [3.0, 2.0]
    direct = adj_loss.binary_loss(res["gnn_output"], graph, distance_fn=tr.distance_fn, grad="sum", grad_params=True)
    assert torch.equal(tr.grad[-2:], direct["grad_params"]) and torch.equal(res["grad_params"], direct["grad_params"])
    assert torch.equal(res["grad_nodes"], direct["grad_nodes"]) and float(direct["grad_params"].abs().min()) > 0.0
    before, g = tr.theta[-2:].cpu().numpy().astype(np.float64), tr.grad[-2:].cpu().numpy().astype(np.float64)
    lr = tr.current_learning_rate()
    tr.apply_gradients()
    want, _, _ = adam_step(before, g, np.zeros(2), np.zeros(2), 1, lr, beta1=0.9, beta2=0.999)
    got = tr.theta[-2:].cpu().numpy().astype(np.float64)
    print(f"[distance] one step: temp, shift {before} -> {got}, float64 Adam {want}")
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all() and (got != before).all()
    assert tr.distance_fn.values() == (float(got[0]), float(got[1]))
    for _ in range(9):
        res = tr.step(graph)
    torch.cuda.synchronize()
    temp, shift = tr.distance_fn.values()
    assert np.isfinite(float(res["sum_loss"])) and abs(temp - 3.0) > 0.02 and abs(shift - 2.0) > 0.02 and tr.global_step == 10
    # the saved state carries them through theta
    state = encoder_trainer_state(tr)
    other = EncoderTrainer(_encoder(G.E2E_CASE, G.e2e_params()), lr=1e-2, num_train_iters=20,
                           distance_fn=adj_loss.TunedSigmoidL2(10.0, 1.0), tune_sigmoid=True)
    other.loss_and_grads(graph)
    assert other.distance_fn.values() == (10.0, 1.0)
    load_encoder_trainer_state(other, state)
    assert other.distance_fn.values() == (temp, shift) and torch.equal(other.theta, tr.theta) and other.global_step == 10
    a, b = tr.step(graph), other.step(graph)
    torch.cuda.synchronize()
    assert torch.equal(a["sum_loss"], b["sum_loss"]) and torch.equal(tr.theta, other.theta)


# ---- 5. the example ------------------------------------------------------------------------------------------------------------
def test_the_example_tunes_the_sigmoid_and_its_encoder_file_names_the_distance(tmp_path):
    from gnf_amd import datasets
    path = str(tmp_path / "encoder.npz")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_gnn.py"), "--dataset", "graph_rnn_grid_small",
                          "--node_embedding_dim", "6", "--latent_dim", "16", "--num_layers", "2", "--num_processing_steps", "2",
                          "--train_batch_size", "4", "--num_train_iters", "3", "--log_every_n_steps", "1",
                          "--eval_every_n_steps", "2", "--binary_dist_fn", "sigmoid_l2", "--tune_sigmoid", "--gaussian_scale", "0.3",
                          "--lr", "0.01", "--save_path", path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "iteration num: 2" in run.stdout and "eval sum loss:" in run.stdout and "after 3 steps" in run.stdout
    logged = re.findall(r"^(?:final )?temp: (\S+) shift: (\S+)$", run.stdout, flags=re.M)
    assert len(logged) == 4, run.stdout[-2000:]               # one per logged iteration, and the final one
    temp, shift = float(logged[-1][0]), float(logged[-1][1])
    assert logged[-1] == logged[-2] and (temp, shift) != (10.0, 1.0)
    enc, hp = encoder.load_encoder(path)
    assert hp["distance"] == {"kind": "sigmoid_l2", "temp": temp, "shift": shift}
    tok = encoder.distance_of(hp)
    assert isinstance(tok, adj_loss.sigmoid_l2) and (tok.temp, tok.shift) == (temp, shift)
    graph = datasets.GraphDataset("graph_rnn_grid_small", 6, 0.3, seed=1).get_random_test_batch(4, torch.device(DEV))
    ev = encoder.evaluate(enc, graph, distance_fn=tok)
    dec = flow.decode_graphs(ev["gnn_output"], distance_fn=tok)
    n = int(graph.nodes.shape[0])
    assert 0 <= int(dec["total_edges"]) <= n * n and dec["graph"].senders.numel() == int(dec["total_edges"])
    # what decode_graphs decodes is what the loss counted: every wrong ordered pair is an edge on one side only
    blocks = flow.pred_adj(ev["gnn_output"], distance_fn=tok)
    assert sum(int((b > 0.5).sum()) for b in blocks) == int(dec["total_edges"])
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_gnn.py"), "--tune_sigmoid", "--num_train_iters", "1"],
                             capture_output=True, text=True, timeout=120)
    assert refused.returncode != 0 and "sigmoid_l2" in refused.stderr
