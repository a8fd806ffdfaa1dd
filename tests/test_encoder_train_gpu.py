"""The encoder's training step on the device (include/gnf_timestep_gnn_train.h): gnn.TimestepGNN.forward_train / backward,
train.EncoderTrainer and examples/run_gnn.py.

Bitwise where the header promises bits: the training forward against gnf_timestep_gnn_f32(is_training = 1), two backward
calls, a backward call without g_x, a captured loss_and_grads replayed.  Every other comparison is with the float64 autograd
restatement (tests/timestep_gnn_grad_ref.py) under one rule per gradient tensor: the larger of the project's gradient rule
(_check_grads of tests/test_train_gpu.py at scale 1e-3: 1e-3 max|ref| + 1e-5 + 1e-6 gmax) and 4 x what the float32
restatement itself differs from float64 by on that tensor.  The inputs of every whole-module case satisfy the restatement's
seed condition (tests/test_encoder_train_cpu.py), so no element is left out.  Every figure is printed before it is asserted
(pytest -s).

Measured on the MI355X, worst ratio (device error / bound) over the gradient tensors of a case; no bound was changed.
  avg_D6_K1_T3_res 0.000            avg_D100_K2_T3_bn_shared 0.001     avg_D6_K3_T1_ln_res 0.000       avg_D100_K3_T3_bn_ln_res_shared 0.001
  avg_D6_K2_T3_bn 0.042             avg_D100_K1_T1 0.000               avg_D6_K2_T3_ln_shared 0.001    sumcat_D100_K1_T3_bn_ln 0.035
  sumcat_D6_K2_T3_res_shared 0.000  sumcat_D100_K3_T1_bn_res 0.001     sumcat_D6_K3_T3_ln_shared 0.001 sumcat_D100_K2_T3_bn_ln_res 0.064
  sumcat_D6_K1_T1_bn 0.000          sumcat_D6_K2_T3_bn_res_shared 0.000  sum_D6_K2_T3_bn_ln_res 0.065  meancat_D100_K3_T3_bn_shared 0.001
  norm stage (BN, LN, BN + LN), rows n, columns D =     1     2     6    64   100   257
    n = 17 (5 + 1 + 11)                      0.000 0.231 0.023 0.024 0.004 0.004
    n = 1                                    0.003 0.059 0.113 0.203 0.052 0.514
    n = 32                                   0.004 0.193 0.027 0.068 0.004 0.018
    n = 33                                   0.061 0.023 0.050 0.026 0.029 0.005
    n = 513                                  0.006 0.974 0.063 0.011 0.041 0.020
  (largest: the batch norm's dbeta of BN + LN at n = 513, D = 2, error 1.46 against 1.49 = 4 x the float32 restatement's own
  0.37 - one of the two features is constant, the layer norm's row variance is near 0: the forward's worst case too)
  tied unshared sum / shared run avg_D100_K2_T3_bn_shared: 0.001 / 0.001
  strided sumcat_D100_K2_T3_bn_ln_res: 0.064
  end to end, hard / soft labels / another true graph (0 of 1570 pairs inside the clip): 0.040 / 0.034 / 0.025"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gnf_amd import _abi, encoder, gnn
from gnf_amd.graphs import csr_desc, csr_of
from gnf_amd.train import EncoderTrainer, encoder_trainer_state, load_encoder_trainer_state
from helpers import GuardBanded, graph_from_arrays

import timestep_gnn_grad_ref as G
import timestep_gnn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(batch, x):
    nn, ne, s, r = batch
    return graph_from_arrays(nn, ne, s, r, x, DEV)


def _encoder(c, params=None):
    return encoder.make_encoder(G.family_hp(c)).set_params(G.make_params(c) if params is None else params)


def _flat_dev(grads, gx=None):
    cp = lambda t: t.detach().cpu().numpy()
    host = {"nets": [[(cp(w), cp(b)) for (w, b) in net] for net in grads["nets"]]}
    for key in ("bn", "ln"):
        if key in grads:
            host[key] = [{k: cp(v) for k, v in d.items()} for d in grads[key]]
    return G.flatten(host, None if gx is None else cp(gx))


def _run(enc, graph, g_out, want_x=True):
    d = graph.nodes.shape[1]
    out, stash = enc.forward_train(graph)
    grads = enc.make_grads(d, torch.device(DEV))
    gx = enc.backward(graph, stash, torch.as_tensor(g_out).to(DEV), grads, want_grad_x=want_x)
    torch.cuda.synchronize()
    return out, grads, gx


def _finish(title, got, r64, r32):
    worst, bad = G.compare(title, got, r64, r32)
    assert not bad, title + "\n" + "\n".join(bad)
    return worst


# ---- 1. whole-module gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GRAD_CASES, ids=R.case_id)
def test_gradients_against_float64_autograd(c):
    seed, x, r64, r32 = G.pick_seed(c)
    assert seed is not None
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    enc = _encoder(c)
    out, grads, gx = _run(enc, graph, G.upstream(x.shape[0], c.d))
    assert torch.equal(graph.nodes, torch.as_tensor(x).to(DEV))
    assert float(np.abs(out.nodes.cpu().numpy() - r64["out"]).max()) <= R.z_bound(r64["out"], r32["out"])
    _finish(R.case_id(c), _flat_dev(grads, gx), r64, r32)


# ---- 2. the norm stage's backward alone ------------------------------------------------------------------------------------------
NORM_SIZES = {"b5_1_11": [5, 1, 11], "n1": [1], "n32": [32], "n33": [33], "n513": [513]}
NORM_WIDTHS = (1, 2, 6, 64, 100, 257)
IDENTITY_KW = dict(agg="sum", combine="agg", epsilon=1.0, activation="relu")


@pytest.mark.parametrize("d", NORM_WIDTHS)
@pytest.mark.parametrize("sizes", list(NORM_SIZES), ids=list(NORM_SIZES))
def test_norm_stage_backward_against_float64(sizes, d):
    from functools import partial
    sizes = NORM_SIZES[sizes]
    n = sum(sizes)
    x = R.norm_inputs(n, d)
    batch = R.edgeless_batch(sizes)
    graph = _graph(batch, x)
    g_out = G.upstream(n, d, seed=d)
    worst = 0.0
    for bn, ln in ((True, False), (False, True), (True, True)):
        tag = ("bn" if bn else "") + ("+" if bn and ln else "") + ("ln" if ln else "")
        rng = np.random.default_rng(100 * d + n)
        p = {"nets": [R.identity_net(d)]}
        if bn:
            p["bn"] = R.make_bn_params(rng, d, 1)
        if ln:
            p["ln"] = R.make_ln_params(rng, d, 1)
        mk = partial(gnn.sum_then_mlp_gnn, partial(gnn.make_mlp_model, 8, d, 1, gnn.relu), 1.0)
        enc = gnn.TimestepGNN(mk, 1, use_batch_norm=bn, residual=False, use_layer_norm=ln).set_params(p)
        r64, r32 = (G.train_step(batch, x, p, 1, dt, IDENTITY_KW, False, False, g_out=g_out) for dt in (np.float64, np.float32))
        out, grads, gx = _run(enc, graph, g_out)
        if n == 1 and bn:
            assert float(gx.abs().max()) == 0.0          # one row: the batch norm's output does not depend on it
        worst = max(worst, _finish(f"norm n={n} D={d} {tag}", _flat_dev(grads, gx), r64, r32))
    print(f"[encoder-train] norm n={n} D={d}: worst ratio {worst:.3f}")


# ---- 3. bit-level checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [G.GRAD_CASES[3], G.GRAD_CASES[0]], ids=R.case_id)   # BN + LN, shared, residual | no norms
def test_train_forward_is_the_training_forward_bit_for_bit(c):
    seed, x, r64, r32 = G.pick_seed(c)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    plain, train = _encoder(c), _encoder(c)
    for _ in range(2):
        a = plain(graph, True).nodes
        b, stash = train.forward_train(graph)
        torch.cuda.synchronize()
        assert torch.equal(a, b.nodes)
        for p, t in zip(plain.bns, train.bns):
            for k in ("batch_mean", "batch_variance", "moving_mean", "moving_variance"):
                assert torch.equal(getattr(p, k), getattr(t, k)), k
    if c.bn:
        assert not np.array_equal(train.bns[0].moving_mean.cpu().numpy(), G.make_params(c)["bn"][0]["moving_mean"])
        assert (train.last_batch_moments is not None) and float(train.bns[0].batch_variance.min()) > 0


@pytest.mark.parametrize("c", [G.GRAD_CASES[3], G.GRAD_CASES[8]], ids=R.case_id)
def test_two_backward_calls_give_the_same_bits_and_g_x_is_optional(c):
    seed, x, r64, r32 = G.pick_seed(c)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    enc = _encoder(c)
    g_out = torch.as_tensor(G.upstream(x.shape[0], c.d)).to(DEV)
    g_before = g_out.clone()
    out, stash = enc.forward_train(graph)
    runs = []
    for want in (True, True, False):
        grads = enc.make_grads(c.d, torch.device(DEV))
        gx = enc.backward(graph, stash, g_out, grads, want_grad_x=want)
        torch.cuda.synchronize()
        runs.append((_flat_dev(grads), gx))
    assert runs[2][1] is None and torch.equal(runs[0][1], runs[1][1]) and torch.equal(g_out, g_before)
    for k, v in runs[0][0].items():
        assert np.array_equal(v, runs[1][0][k]) and np.array_equal(v, runs[2][0][k]), k
        assert np.isfinite(v).all()


# ---- 4. weight sharing ---------------------------------------------------------------------------------------------------------------
def test_shared_net_gradients_are_the_sum_over_timesteps():
    c = G.GRAD_CASES[1]                                   # avg D 100 K 2 T 3 BN, shared
    assert c.sharing and c.t == 3
    seed, x, r64, r32 = G.pick_seed(c)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    g_out = G.upstream(x.shape[0], c.d)
    p = G.make_params(c)
    tied = dict(p, nets=[p["nets"][0]] * c.t)
    _, gs, gxs = _run(_encoder(c, p), graph, g_out)
    _, gu, gxu = _run(_encoder(c._replace(sharing=False), tied), graph, g_out)
    summed = {"nets": [[(sum(gu["nets"][q][j][0] for q in range(c.t)), sum(gu["nets"][q][j][1] for q in range(c.t)))
                        for j in range(c.k)]], "bn": gu["bn"]}
    _finish("tied sum " + R.case_id(c), _flat_dev(summed, gxu), r64, r32)
    _finish("shared " + R.case_id(c), _flat_dev(gs, gxs), r64, r32)
    per_step = gu["nets"][0][0][0].cpu().numpy()          # one timestep's share alone is far from the sum
    assert np.abs(per_step - r64["grads"]["nets"][0][0][0]).max() > 10 * G.bounds(r64, r32)["net0.W0"]


# ---- 5. strides (raw entry points) -----------------------------------------------------------------------------------------------------
def _raw_forward(enc, desc, csr, x_ptr, ldx, out_ptr, ldo, n, d, stash=None, stash_bytes=None, ws_bytes=None):
    lib = _abi.lib()
    need_ws, need_st = lib.gnf_timestep_gnn_workspace_bytes(n, d, C.byref(desc)), lib.gnf_timestep_gnn_stash_bytes(n, d, C.byref(desc))
    ws = torch.empty(max(need_ws, 8), dtype=torch.uint8, device=DEV)
    stash = torch.empty(max(need_st, 8), dtype=torch.uint8, device=DEV) if stash is None else stash
    rc = lib.gnf_timestep_gnn_train_forward_f32(C.byref(csr), C.byref(desc), x_ptr, ldx, out_ptr, ldo, d, _abi.ptr(stash),
                                                need_st if stash_bytes is None else stash_bytes, _abi.ptr(ws),
                                                need_ws if ws_bytes is None else ws_bytes, _abi.stream_ptr(torch.device(DEV)))
    return rc, stash, need_st


def _raw_backward(desc, gdesc, csr, csr_t, x_ptr, ldx, g_ptr, ldg, gx_ptr, ldgx, n, d, stash, stash_bytes, ws_bytes=None):
    lib = _abi.lib()
    need = lib.gnf_timestep_gnn_backward_workspace_bytes(n, d, C.byref(desc))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    return lib.gnf_timestep_gnn_backward_f32(C.byref(csr), C.byref(csr_t) if csr_t is not None else None, C.byref(desc),
                                             C.byref(gdesc) if gdesc is not None else None, x_ptr, ldx, g_ptr, ldg, gx_ptr, ldgx, d,
                                             _abi.ptr(stash), stash_bytes, _abi.ptr(ws), need if ws_bytes is None else ws_bytes,
                                             _abi.stream_ptr(torch.device(DEV)))


def test_strided_x_g_out_and_g_x_leave_guard_bands_and_inputs_untouched():
    c = G.GRAD_CASES[11]                                  # sumcat D 100 K 2 T 3 BN + LN, residual
    seed, x, r64, r32 = G.pick_seed(c)
    n, d = x.shape
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    enc = _encoder(c)
    dev = torch.device(DEV)
    desc, keep = enc._desc(d, dev, True)
    grads = enc.make_grads(d, dev)
    gdesc, gkeep = enc._grad_desc(grads, d, dev)
    csr, csr_t = csr_desc(graph, csr_of(graph), False), csr_of(graph, by_sender=True).desc
    xin = GuardBanded(n, d, d + 9, c0=3, device=DEV, fill=x)
    out = GuardBanded(n, d, d + 5, c0=1, device=DEV)
    gout = GuardBanded(n, d, d + 7, c0=2, device=DEV, fill=G.upstream(n, d))
    gx = GuardBanded(n, d, d + 3, c0=1, device=DEV)
    x_before, g_before = xin.bits.clone(), gout.bits.clone()
    rc, stash, st_bytes = _raw_forward(enc, desc, csr, xin.ptr(), xin.ld, out.ptr(), out.ld, n, d)
    assert rc == 0, _abi.lib().gnf_last_error()
    rc = _raw_backward(desc, gdesc, csr, csr_t, xin.ptr(), xin.ld, gout.ptr(), gout.ld, gx.ptr(), gx.ld, n, d, stash, st_bytes)
    assert rc == 0, _abi.lib().gnf_last_error()
    torch.cuda.synchronize()
    out.check_guard(), gx.check_guard()
    assert torch.equal(xin.bits, x_before) and torch.equal(gout.bits, g_before)
    got = _flat_dev(grads)
    got["g_x"] = gx.numpy()
    _finish("strided " + R.case_id(c), got, r64, r32)
    # g_x overlapping g_out is refused before any launch
    rc = _raw_backward(desc, gdesc, csr, csr_t, xin.ptr(), xin.ld, gout.ptr(), gout.ld,
                       C.c_void_p(gout.ptr().value + 4 * gout.ld * (n - 1)), gout.ld, n, d, stash, st_bytes)
    assert rc == -1 and "overlap" in _abi.lib().gnf_last_error().decode()
    assert torch.equal(gout.bits, g_before)


# ---- 6. end to end: EncoderTrainer.loss_and_grads ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.E2E_KINDS)
def test_loss_and_grads_against_binary_loss_behind_the_reference(kind):
    seed, x, r64, r32 = G.pick_e2e(kind)
    assert seed is not None and r64["clipped"] <= 8
    c, loss = G.E2E_CASE, G.e2e_loss(kind)
    batch = R.ring_chord_batch(R.SIZES)
    graph = _graph(batch, x)
    true_graph = _graph((batch[0], loss["n_edge"], loss["senders"], loss["receivers"]), x) if kind == "other" else None
    tr = EncoderTrainer(_encoder(c, G.e2e_params()), use_soft_labels=loss["soft"])
    res = tr.loss_and_grads(graph, true_graph)
    torch.cuda.synchronize()
    got = G.flatten(tr.named_gradients())
    sum_loss = float(res["sum_loss"])
    print(f"[encoder-train] e2e {kind}: sum_loss {sum_loss:.6f} reference {r64['sum_loss']:.6f}")
    # 1570 softplus terms, each an fp32 value of a logit the encoder's fp32 output moves by < 1e-3 (CLIP_GAP's reasoning)
    assert abs(sum_loss - r64["sum_loss"]) <= 1e-4 * abs(r64["sum_loss"]) and float(res["total_loss"]) == sum_loss
    _finish(f"e2e {kind}", got, r64, r32)
    assert tr.grad.numel() == sum(v.size for v in got.values())


# ---- 7. optimiser step -----------------------------------------------------------------------------------------------------------------
def _f32_update(moving, batch):
    omd = np.float32(1.0) - np.float32(R.BN_DECAY)
    return (moving - ((moving - batch).astype(np.float32) * omd).astype(np.float32)).astype(np.float32)


def _host_adam(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, epsilon=1e-8):
    """oracle.gnf_oracle.adam_step in float64 with the two decay rates as gnf_adam_f32 receives them: C floats.  The step size
    lr_t comes from the exact rates on the host, as the trainer (and TensorFlow's python side) forms it; 1 - float32(0.999)
    is 1.3e-5 below 1e-3 in relative terms, which the second moment carries whole (at run_grevnet.py's beta2 = 0.9 of the
    Adam-step test in tests/test_train_gpu.py the same effect is 2.4e-7 and inside its tolerances)."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return w - lr_t * m / (np.sqrt(v) + epsilon), m, v


def test_three_adam_steps_follow_a_float64_host_adam_fed_the_devices_gradients():
    c = G.E2E_CASE
    seed, x, _, _ = G.pick_e2e("hard")
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    p = G.e2e_params()
    tr = EncoderTrainer(_encoder(c, p), lr=1e-2, num_train_iters=4)
    moving = [(b["moving_mean"], b["moving_variance"]) for b in p["bn"]]
    w = m = v = None
    for t in (1, 2, 3):
        lr = tr.current_learning_rate()
        assert math.isclose(lr, (1e-2 - 1e-4) * math.sqrt(1.0 - (t - 1) / 4.0) + 1e-4, rel_tol=1e-14)   # polynomial_decay
        tr.loss_and_grads(graph)
        if w is None:
            w, m, v = tr.theta.cpu().numpy().astype(np.float64), np.zeros(tr.theta.numel()), np.zeros(tr.theta.numel())
        g = tr.grad.cpu().numpy().astype(np.float64)
        batch = [(b.batch_mean.cpu().numpy().copy(), b.batch_variance.cpu().numpy().copy()) for b in tr.net.bns]
        tr.apply_gradients()
        w, m, v = _host_adam(w, g, m, v, t, lr)
        moving = [(_f32_update(mm, bm), _f32_update(mv, bv)) for (mm, mv), (bm, bv) in zip(moving, batch)]
        torch.cuda.synchronize()
        # the comparison rule of the Adam-step test in tests/test_train_gpu.py
        np.testing.assert_allclose(tr.theta.cpu().numpy(), w, rtol=2e-6, atol=2e-6)
        # the moments (not part of that rule: its gradient is the same every step, here it changes sign, so m is a difference
        # of terms up to max|g| and carries their fp32 rounding): t steps of three fp32 operations on terms of that size
        gm = float(np.abs(g).max())
        np.testing.assert_allclose(tr.m.cpu().numpy(), m, rtol=2e-6, atol=3 * t * 2.0 ** -24 * gm)
        np.testing.assert_allclose(tr.v.cpu().numpy(), v, rtol=2e-6, atol=3 * t * 2.0 ** -24 * gm * gm)
    assert tr.global_step == 3
    for b, (mm, mv) in zip(tr.net.bns, moving):           # the moving statistics advanced exactly three times
        assert np.array_equal(b.moving_mean.cpu().numpy(), mm) and np.array_equal(b.moving_variance.cpu().numpy(), mv)
    # the encoder reads the arena: its parameters are the updated ones, and a saved / restored state resumes
    assert np.array_equal(tr.net.get_params()["nets"][0][0][0].ravel(), tr.theta[:tr.net.get_params()["nets"][0][0][0].size].cpu().numpy())
    state = encoder_trainer_state(tr)
    tr.step(graph)
    after = tr.theta.clone()
    load_encoder_trainer_state(tr, state)
    assert tr.global_step == 3
    tr.step(graph)
    torch.cuda.synchronize()
    assert torch.equal(tr.theta, after)


# ---- 8. capture ----------------------------------------------------------------------------------------------------------------------
def test_a_captured_loss_and_grads_replayed_equals_eager_steps_bit_for_bit():
    """The captured region is loss_and_grads (train-forward, loss, backward: every launch but one); the Adam launch takes its
    step size by value and the step size changes every step, so apply_gradients runs eagerly behind each replay."""
    c = G.E2E_CASE
    seed, x, _, _ = G.pick_e2e("hard")
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    eager = EncoderTrainer(_encoder(c, G.e2e_params()), lr=1e-2, num_train_iters=4, max_nodes_per_graph=64)
    want = []
    for _ in range(2):
        res = eager.step(graph)
        torch.cuda.synchronize()
        want.append((eager.theta.clone(), eager.grad.clone(), res["sum_loss"].clone(), eager.net.bns[0].moving_mean.clone()))
    assert not torch.equal(want[0][0], want[1][0])
    tr = EncoderTrainer(_encoder(c, G.e2e_params()), lr=1e-2, num_train_iters=4, max_nodes_per_graph=64)
    tr.loss_and_grads(graph)                                # variables, CSRs and the allocator's blocks exist
    for b, q in zip(tr.net.bns, G.e2e_params()["bn"]):      # ... and the warm-up's moving-average update is taken back
        b.moving_mean.copy_(torch.as_tensor(q["moving_mean"])), b.moving_variance.copy_(torch.as_tensor(q["moving_variance"]))
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        res_c = tr.loss_and_grads(graph)
    for k in range(2):
        tr.grad.zero_()
        cg.replay()
        tr.apply_gradients()
        torch.cuda.synchronize()
        theta, grad, loss, mm = want[k]
        assert torch.equal(res_c["sum_loss"], loss) and torch.equal(tr.grad, grad) and torch.equal(tr.theta, theta), k
        assert torch.equal(tr.net.bns[0].moving_mean, mm), k


# ---- 9. rejections (raw entry points) -----------------------------------------------------------------------------------------------
def _setup(c, enc=None, is_training=True):
    x = R.module_inputs(c, 0)
    n, d = x.shape
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    enc = _encoder(c) if enc is None else enc
    dev = torch.device(DEV)
    desc, keep = enc._desc(d, dev, is_training)
    csr = csr_desc(graph, csr_of(graph), enc.blocks()[0].graph_scope)
    csr_t = csr_of(graph, by_sender=True).desc
    xin = torch.as_tensor(x).to(DEV)
    return dict(enc=enc, graph=graph, desc=desc, keep=keep, csr=csr, csr_t=csr_t, x=xin, n=n, d=d)


@pytest.mark.parametrize("family", ["dm", "graph"])
def test_attention_nets_are_unsupported_before_any_launch(family):
    c = R.Case(family, 6, 32, 2, 2, True, False, True, False)
    enc = encoder.make_encoder(R.family_hp(c)).set_params(R.make_params(c))
    s = _setup(c, enc)
    n, d = s["n"], s["d"]
    out = torch.full((n, d), 7.0, device=DEV)
    stash = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    moving = enc.bns[0].moving_mean.clone()
    rc, _, _ = _raw_forward(enc, s["desc"], s["csr"], _abi.ptr(s["x"]), d, _abi.ptr(out), d, n, d, stash=stash, stash_bytes=1 << 16)
    msg = _abi.lib().gnf_last_error().decode()
    assert rc == -5 and "attention" in msg, msg
    gx = torch.full((n, d), 7.0, device=DEV)
    gdesc = s["desc"]                                        # (refused before grad is looked at)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    rc = _abi.lib().gnf_timestep_gnn_backward_f32(C.byref(s["csr"]), C.byref(s["csr_t"]), C.byref(s["desc"]), C.byref(gdesc),
                                                  _abi.ptr(s["x"]), d, _abi.ptr(out), d, _abi.ptr(gx), d, d, _abi.ptr(stash), 1 << 16,
                                                  _abi.ptr(ws), 1 << 16, _abi.stream_ptr(torch.device(DEV)))
    msg = _abi.lib().gnf_last_error().decode()
    assert rc == -5 and "attention" in msg, msg
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max()) and float(gx.min()) == 7.0 and torch.equal(enc.bns[0].moving_mean, moving)
    with pytest.raises(_abi.GnfError, match="attention"):
        enc.forward_train(s["graph"])


def test_invalid_calls_give_their_codes():
    c = G.GRAD_CASES[4]                                     # avg D 6 K 2 T 3 BN
    s = _setup(c)
    enc, n, d, dev = s["enc"], s["n"], s["d"], torch.device(DEV)
    lib = _abi.lib()
    out = torch.full((n, d), 7.0, device=DEV)
    xp, op = _abi.ptr(s["x"]), _abi.ptr(out)
    # is_training = 0
    desc_eval, keep_eval = enc._desc(d, dev, False)
    rc, _, _ = _raw_forward(enc, desc_eval, s["csr"], xp, d, op, d, n, d)
    assert rc == -1 and "is_training" in lib.gnf_last_error().decode()
    # short ws, short stash
    rc, _, need_st = _raw_forward(enc, s["desc"], s["csr"], xp, d, op, d, n, d, ws_bytes=64)
    assert rc == -3 and "workspace" in lib.gnf_last_error().decode()
    rc, _, _ = _raw_forward(enc, s["desc"], s["csr"], xp, d, op, d, n, d, stash_bytes=need_st - 1)
    assert rc == -3 and "stash" in lib.gnf_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())
    rc, stash, st_bytes = _raw_forward(enc, s["desc"], s["csr"], xp, d, op, d, n, d)
    assert rc == 0
    grads = enc.make_grads(d, dev)
    for net in grads["nets"]:
        for w, b in net:
            w.fill_(7.0), b.fill_(7.0)
    gdesc, gkeep = enc._grad_desc(grads, d, dev)
    g = torch.ones((n, d), device=DEV)
    args = (xp, d, _abi.ptr(g), d, None, d, n, d)
    assert _raw_backward(desc_eval, gdesc, s["csr"], s["csr_t"], *args, stash, st_bytes) == -1
    assert _raw_backward(s["desc"], gdesc, s["csr"], s["csr_t"], *args, stash, st_bytes, ws_bytes=64) == -3
    assert _raw_backward(s["desc"], gdesc, s["csr"], s["csr_t"], *args, stash, st_bytes - 1) == -3
    assert _raw_backward(s["desc"], gdesc, s["csr"], None, *args, stash, st_bytes) == -1
    assert _raw_backward(s["desc"], None, s["csr"], s["csr_t"], *args, stash, st_bytes) == -1
    assert _raw_backward(s["desc"], gdesc, s["csr"], s["csr_t"], xp, d, None, d, None, d, n, d, stash, st_bytes) == -1
    other = _encoder(c._replace(t=2))                       # a grad of another shape: T = 2
    odesc, okeep = other._grad_desc(other.make_grads(d, dev), d, dev)
    assert _raw_backward(s["desc"], odesc, s["csr"], s["csr_t"], *args, stash, st_bytes) == -1
    assert "shape" in lib.gnf_last_error().decode()
    torch.cuda.synchronize()
    assert all(float(w.min()) == 7.0 and float(b.max()) == 7.0 for net in grads["nets"] for w, b in net)   # nothing was launched
    # n_nodes == 0: GNF_OK, every gradient buffer zeroed
    rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    col = torch.zeros(1, dtype=torch.int32, device=DEV)
    empty = _abi.GnfCsr(rowptr.data_ptr(), col.data_ptr(), 0, 0, None, 0)
    rc = _raw_backward(s["desc"], gdesc, empty, empty, None, d, None, d, None, d, 0, d, stash, st_bytes)
    assert rc == 0, lib.gnf_last_error()
    torch.cuda.synchronize()
    flat = _flat_dev(grads)
    assert all(float(np.abs(v).max()) == 0.0 for v in flat.values()) and len(flat) == 2 * c.k * c.t + 2 * c.t


def test_cpu_tensors_raise():
    c = G.GRAD_CASES[4]
    x = R.module_inputs(c, 0)
    nn, ne, s, r = R.ring_chord_batch(R.SIZES)
    cpu_graph = graph_from_arrays(nn, ne, s, r, x, "cpu")
    with pytest.raises(_abi.GnfError):
        _encoder(c).forward_train(cpu_graph)
    with pytest.raises(_abi.GnfError):
        EncoderTrainer(_encoder(c)).loss_and_grads(cpu_graph)


# ---- 10. the example -----------------------------------------------------------------------------------------------------------------
def test_the_example_trains_and_saves_an_encoder_load_encoder_reads_back(tmp_path):
    path = str(tmp_path / "encoder.npz")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_gnn.py"), "--dataset", "graph_rnn_grid_small",
                          "--node_embedding_dim", "6", "--latent_dim", "16", "--num_layers", "2", "--num_processing_steps", "2",
                          "--train_batch_size", "4", "--num_train_iters", "3", "--log_every_n_steps", "1",
                          "--eval_every_n_steps", "2", "--save_path", path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "iteration num: 2" in run.stdout and "eval sum loss:" in run.stdout and "after 3 steps" in run.stdout
    enc, hp = encoder.load_encoder(path)
    assert hp["node_dim"] == 6 and hp["num_timesteps"] == 2 and enc.weight_sharing and enc.use_batch_norm
    p = enc.get_params()
    assert len(p["nets"]) == 1 and p["nets"][0][0][0].shape == (6, 16) and len(p["bn"]) == 2
    # trained: three Adam steps moved gamma off its initial ones and the moving statistics off theirs
    assert not np.array_equal(p["bn"][0]["gamma"], np.ones(6, np.float32)) and not np.array_equal(p["bn"][0]["moving_mean"], np.zeros(6, np.float32))
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_gnn.py"), "--dataset", "graph_rnn_grid_small",
                              "--attn_type", "dm_attn", "--node_embedding_dim", "6", "--latent_dim", "16", "--num_layers", "2",
                              "--num_processing_steps", "2", "--train_batch_size", "4", "--num_train_iters", "1", "--save_path", path],
                             capture_output=True, text=True, timeout=120)
    assert refused.returncode != 0 and "attention" in refused.stderr
