"""The batch-norm bijector on every route the library has for it, at the widths and row counts where the route changes.

The bijector's two-level fp64 reduction of [parts][H][2] partial rows exists many times over in csrc/ (k_bn_stats /
k_bn_apply, the column sums of the fused forward kernel and of k_coupling_rows, the bijector on load of the attention
instance + k_bn_affine, k_bn_denorm and the deferred inverse of k_half_fused, k_bn_bwd_stats / k_bn_bwd_apply, the rows
k_attn_bwd_dx_mfma leaves, the fold into the fused backward prologue, k_bn_post_step); which copy runs is decided in
grevnet_walk (gnf_abi.hip) and the backward walk (gnf_train.hip) from H, n, the net kind, net.fused and the number of
partial rows the previous kernel left.  Each table below names, from that dispatch code, the route every shape takes.

Reference: oracle/gnf_oracle.py in float64 (loss_and_grads; Fp64Dense.f's last_bn_moments; Fp64Dense.g).  Inputs carry
three hard columns per half (batch_norm_routes.hard_nodes), nets are built with final_scale = 0.05.  Every bound is the
larger of the project's bound for that quantity (z, g(zs): 5e-4 max(1, |ref|max); loss: 1e-4 per node; gradients:
3e-4 max|g| + 1e-5 + 1e-6 gmax; gamma / beta gradients: 3e-4 max|g| + 1e-4; batch moments: 3e-5, + 3e-5 relative for the
variance) and 4 x what the oracle's own float32 run differs from its float64 run by on the same inputs (the device sums
in another order and uses expf / sqrtf).  No bound comes from the code under test.  Two notes on the float32 half:
  * batch moments: each bijector's own float32 deviation - below n = 15 the largest over the case's bijectors (the same
    arithmetic on columns of the same kind), where a single bijector's figure is one or two roundings and says little -
    D34_n2, bijector (1, 1): the float32 oracle happens to be 6.4e-6 off, the device 2.5e-4, the float32 oracle at bijector (0, 1) of the same case
    1.7e-4 (y = x * scale + shift, the reference's form, rounds x * scale where it is ~2000 for the 100 + 0.1 N column);
  * gradients: a hidden unit whose pre-activation is within rounding of its relu's kink takes either side in float32 and
    a whole term of the gradient comes or goes with it (attn_D34_n528: one unit of t[1][1] at -2.5e-6, every tensor in
    front of it 1e-2 off on both paths alike).  check_grads therefore compares a missing case once more against float64
    autograd that takes the device's side for the units inside the oracle's own kink band, and only for those.

Measured on an MI355X, with the float32 oracle run on that machine's CPU, as printed by `pytest -s`; 91 tests, 28 s
(each pair: float32 oracle / device, both against the float64 oracle; the case of the family that comes closest to its bound;
gradient errors are absolute, with the bound they were held to in brackets)
message passing (28 cases): z 1.3e-4 / 9.5e-5; loss 8.6e-4 / 1.0e-3 (n = 33); mean 2.0e-5 / 4.3e-5; var 6.1e-6 / 9.6e-6;
    g(zs) 4.5e-6 / 3.7e-6; reconstruction 3.6e-7; gradients 2.6e-4 / 6.6e-3 (bound 1.1e-2); gamma, beta 1.0e-5 / 5.8e-5 (1.8e-4)
wide layered (6): z 7.1e-5 / 1.4e-5; loss 1.5e-3 / 3.4e-3 (n = 531); mean 5.2e-6 / 1.3e-5; var 1.6e-6 / 2.0e-6; g(zs) 5.6e-6 /
    5.9e-6; reconstruction 3.5e-7; gradients 2.1e-4 / 4.8e-3 (1.8e-2); gamma, beta 3.5e-4 / 4.8e-3 (3.3e-2)
1024-row limit (4): z 1.3e-6 / 1.1e-6; loss 6.9e-4 / 3.3e-3 (n = 16384); mean 1.1e-8 / 7.1e-9; var 2.8e-8 / 6.6e-8; g(zs) 5.4e-6
    / 5.0e-6; reconstruction 3.1e-7; gradients 4.9e-4 / 6.7e-4 (5.0e-3); gamma, beta 5.8e-4 / 6.5e-4 (3.7e-3)
tiny batches (24): z 7.0e-5 / 4.7e-5; loss 7.3e-5 / 8.0e-5 (n = 2); mean 1.2e-4 / 2.2e-4 (n = 1); var 1.8e-5 / 1.0e-5; g(zs)
    4.9e-7 / 7.1e-7; reconstruction 2.4e-7; gradients 1.9e-5 / 1.1e-4 (4.8e-4); gamma, beta 2.9e-4 / 2.8e-4 (3.1e-3)
attention (26; the two attn_bwd_rows runs repeat these figures to the digits shown): z 3.8e-4 / 1.5e-4 and loss 1.1e-2 /
    4.5e-3 (layer norm, n = 513); mean 2.1e-5 / 4.6e-5; var 1.1e-5 / 8.0e-6; g(zs) 4.3e-5 / 3.1e-5; reconstruction 7.0e-7;
    gradients 1.2e-4 / 5.1e-3 (7.9e-3); gamma, beta 6.5e-2 / 6.5e-2 (2.6e-1); attn_D34_n528 needed the kink-aware
    comparison: 35 units inside the 4.1e-4 band, one (t[1][1], node 10, unit 15) on the other side on the device, on
    both paths and under both attn_bwd_rows settings; against the float64 sides s[0][0].wk was 2.0e-2 off (bound 1.4e-2)
post-step, T = 25 (1): z 1.7e-6 / 8.0e-7; loss 4.4e-5 / 3.6e-5; mean 1.3e-7 / 6.8e-8; var 7.3e-8 / 1.2e-7; gradients 5.2e-6 /
    4.6e-6 (1.2e-4); gamma, beta 3.3e-6 / 4.4e-6 (2.1e-4); gamma and both moving statistics of all 50 bijectors within their
    elementwise float32 bounds
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_norm_routes as B
from batch_norm_routes import attn, mp
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _check_case(c, fused, grads=True):
    """Plain forward (z, loss, log-det, moments), g(zs), then the training step (the same terms from the training forward,
    the reconstruction, and - when asked - every gradient) against the case's shared reference."""
    ref, pr = B.reference(c), B.problem(c)
    rep = B.Report(f"{B.case_id(c)} {'fused' if fused else 'layered'}")
    fwd = B.run_forward(c, fused)
    B.check_forward_terms(rep, fwd, ref, c.n)
    B.check_inverse(rep, fwd, ref)
    trn = B.run_training(c, fused)
    B.check_forward_terms(rep, trn, ref, c.n, tag="train:")
    B.check_reconstruction(rep, trn, pr["x"])
    if grads:
        B.check_grads(rep, trn, ref, c)
    rep.finish()


# ---- 1. message-passing nets on both paths ---------------------------------------------------------------------------------
MP_CASES = ([mp(d, 513) for d in (2, 6, 200, 256, 258)] + [mp(6, n) for n in (17, 33, 512, 528)] +
            [mp(256, n) for n in (17, 33, 512, 528)] + [mp(258, 528)])


@PATHS
@pytest.mark.parametrize("c", MP_CASES, ids=[B.case_id(c) for c in MP_CASES])
def test_message_passing_routes(c, fused):
    """D = 2, 6, 200, 256, 258 (H = 1, 3, 100, 128, 129) x n = 17, 33, 512, 513, 528 (2, 3, 32, 33, 33 sixteen-row tiles):
    every H at n = 513, every n at H = 3 and H = 128, H = 129 at n = 528.  latent = 16 keeps every width inside
    fused_supported (fused_lds_bytes of the (1, 2) shape: 2 x 2 x 16 rows of pad16(H) + 4 floats), so `fused` is the fused
    path at every H here, H = 129 included.
    Forward, both paths: the first bijector has no predecessor (bn_pre = 0) and runs k_bn_stats (bn_blocks: chunks of at
    least 32 rows, sixteen at most) + k_bn_apply's one-thread-per-column walk.  Every later bijector gets the column sums of
    the half-step in front of it, one row per sixteen-node tile ((n + 15) / 16 <= kBnPartRowsMax, so hs.bn_part is set):
      fused   - k_half_fused<1, 2> (choose_shape: at most one tile per CU), the a.bn_part block behind the coupling; the
                training forward runs its STASH instance (fused_stash_shape), which leaves the same rows;
      layered - k_coupling_rows (launch_coupling: H <= 256), thread (rs, c) with 256 / H row lanes: H = 3, 100 and 129
                leave idle threads, H = 129 has one lane.
    k_bn_apply then walks them grouped (G = 256 / H thread groups) when nparts > 32 && H <= 128: n = 513 and 528 at
    H <= 128 (G = 256, 85, 2, 2: at H = 3 and 100 G * H < 256 and the tail threads sit out), one thread per column at
    n <= 512 (32 rows or fewer) and at H = 129 (33 rows walked serially, eight in flight).
    Inverse: k_bn_denorm after every half-step.  Backward: message-passing nets leave no partial rows (bn_pre is the
    attention backward's), so every bijector runs k_bn_bwd_stats (16 chunks at most: the serial walk) + k_bn_bwd_apply -
    from the merged walk (fused, stash) and from the generic GEMM walk (layered)."""
    _check_case(c, fused)


# ---- 2. widths past the column sums of k_coupling_rows -------------------------------------------------------------------
WIDE_CASES = [mp(d, n) for d in (512, 514, 600) for n in (40, 531)]


@pytest.mark.parametrize("c", WIDE_CASES, ids=[B.case_id(c) for c in WIDE_CASES])
def test_layered_wide_halves(c):
    """net.fused = False, D = 512, 514, 600 (H = 256, 257, 300) at n = 40 and 531 (3 and 34 sixteen-row workgroups).
    H = 256 is the last width launch_coupling hands to k_coupling_rows (H <= 256; one row lane per column, no idle
    thread), whose rows k_bn_apply walks one thread per column (H > 128: G = 1) - 34 of them at n = 531.  H = 257 and 300
    take k_coupling (no sums: *n_bn stays 0), so every bijector runs k_bn_stats, whose second 256-column pass (c0 = 256) is
    1 and 44 columns wide (256 and 5 row lanes); k_bn_apply, k_bn_denorm, k_bn_bwd_stats (the same two passes) and
    k_bn_bwd_apply loop over c = tid, tid + 256."""
    _check_case(c, False)


# ---- 3. the 1024-partial-row limit ----------------------------------------------------------------------------------------------
LIMIT_CASES = [mp(4, 16384), mp(4, 16385)]


@PATHS
@pytest.mark.parametrize("c", LIMIT_CASES, ids=[B.case_id(c) for c in LIMIT_CASES])
def test_partial_row_limit(c, fused):
    """D = 4, n = 16384 / 16385: (n + 15) / 16 = 1024 / 1025 against kBnPartRowsMax = 1024 in grevnet_walk.
    layered: 1024 workgroups of k_coupling_rows fill the moment buffer to its last row and k_bn_apply walks them grouped
    (H = 2: G = 128 thread groups, eight rows each, one round of sixteen slots); at 1025 hs.bn_part stays NULL, k_coupling
    runs and every bijector takes k_bn_stats (bn_blocks: 16 chunks of 1025 rows, the last one 1010).
    fused: at 16384 the both-nets kernel runs 32-row tiles (choose_shape (2, 2): more tiles than CUs; choose_big keeps out
    while ceil(g / 2 CUs) = 2 on a 256-CU device) and leaves 512 rows; at 16385 choose_big takes the large-batch kernel,
    which leaves no sums (a.bn_part = nullptr, *n_bn = 0) - and hs.bn_part is NULL anyway: every bijector runs its own
    moment pass.  The reference's moments and g(zs) come from the float64 gather oracle here (a dense adjacency of
    16385^2 doubles is 2 GB)."""
    _check_case(c, fused)


# ---- 4. tiny batches -----------------------------------------------------------------------------------------------------
TINY_CASES = [mp(d, n) for n in (1, 2, 15, 16) for d in (2, 6, 34)]


@PATHS
@pytest.mark.parametrize("c", TINY_CASES, ids=[B.case_id(c) for c in TINY_CASES])
def test_tiny_batches(c, fused):
    """n = 1, 2, 15, 16 x D = 2, 6, 34: one tile, one partial row (k_bn_stats with a single short chunk for the first
    bijector, one row from k_half_fused / k_coupling_rows for the others), every walk's tail handling with nparts = 1.
    At n = 1 every variance is zero, at any n the constant column's is: q / n - mean^2 may round below zero and must be
    clamped (batch_variance >= 0 exactly, checked by check_forward_terms).  Gradients are compared from n = 15 up: at
    n = 2 the oracle's own float32 run is 5 % off on a gamma gradient through cancellation, a comparison would test
    nothing."""
    _check_case(c, fused, grads=c.n >= 15)


# ---- 5. attention nets, the drivers' geometry ----------------------------------------------------------------------------
@PATHS
@pytest.mark.parametrize("c", B.ATTN_CASES, ids=[B.case_id(c) for c in B.ATTN_CASES])
def test_attention_routes(c, fused):
    """8 heads, kq = v = 10, out 80, no layer norm, sparse edges (ring + random: fewer than 24 per node); D = 2, 34, 64
    (H = 1, 17, 32) x n = 17, 513, 528 (2, 33, 33 sixteen-row tiles).
    fused, forward: grevnet_walk asks fused_bn_on_load_ok once per call.  front_fold_ok wants the layer-0 width and, with
    concat, H itself to be multiples of 16: of the drivers' concat nets only H = 32 folds - there every bijector is
    applied on load (gnf_attn_front_dev.h, bnf block: kFrThreads / H thread groups over the rows k_bn_stats (first
    bijector) or the fused kernel's a.bn_part block (the others) left, ping-ponging between two row buffers) and
    k_bn_affine normalises the last conditioning half.  The two no-concat cases put H = 1 and 17 through the same block
    (layer-0 width 80).  In the training forward the stash instance exists for the fixed geometry only (H = 32): the
    no-concat nets fold in log_prob_terms and take the separate passes in loss_and_grads - both are compared.
    H = 1 and 17 with concat, D = 66 (H = 33: pad16(H) is three fragments, front_fold_ok refuses) and layer_norm = True
    (choose_shape: one net per workgroup; fused_bwd_supported and front_fold_ok refuse) take k_bn_stats / k_bn_apply: the
    fused kernel's rows at NETS = 2, k_coupling_rows' for the layer-norm net.
    fused, inverse: the same answer of fused_bn_on_load_ok defers each bn.forward to the next half-step's kernel
    (bnu_inv) and ends with one k_bn_denorm; elsewhere k_bn_denorm per half-step.
    Backward (both paths): the attention backward's last kernel writes the final dL/dy rows and leaves the bijector's
    (sum G, sum G xh) rows, one per 16 rows (k_attn_bwd_dx_mfma: the walk always packs [Wq | Wk | Wv]^T, so this - not
    k_attn_bwd_dx / k_attn_bwd_dx2 - is the writer at every shape here).  On the merged walk (fused, not layer norm) with
    H <= 128 the bijector is folded into the next half-step's prologue (gnf_fused_bwd_dev.h, bnf block; 2 rows at n = 17,
    33 at 513 / 528), the walk's last one and every one of the other walks go through k_bn_bwd_apply with pre_parts rows
    (grouped walk at 33 rows).
    NOT covered: the a.bn_part blocks of k_attn_bwd_dx and k_attn_bwd_dx2.  launch_attn_backward has one caller (the walk
    of gnf_train.hip), which packs the transposed weights for every edge-scope net (wot_packed) and returns through
    launch_attn_graph_backward for the graph scope (*n_parts = 0: no rows at all); without the packed weights only a
    geometry whose k_attn_bwd_dx_mfma staging passes 160 KB gets there, and validate_attn's row limit (1272 floats) ends
    at 163 328 bytes.  No product object reaches those two blocks, so no case here can.
    layered: launch_attn_pair + the layered MLP + k_coupling_rows' rows for every bijector but the first."""
    _check_case(c, fused)


@pytest.fixture(scope="module")
def _attn_children(tmp_path_factory):
    """One child interpreter per attn_bwd_rows setting (the option reaches it through the binding's GNF_OPTIONS variable,
    as in test_weight_gradient_kernel_launch_shapes, so it cannot leak): the training step of every attention case."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = {}

    def run(rows):
        if rows not in done:
            path = str(tmp_path_factory.mktemp("bn_routes") / f"rows{rows}.npz")
            e = dict(os.environ, GNF_OPTIONS=f"attn_bwd_rows={rows}")
            r = subprocess.run([sys.executable, os.path.join(root, "tests", "batch_norm_routes.py"), path], env=e,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "bn-routes-child-ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
            done[rows] = path
        return done[rows]
    return run


@pytest.mark.parametrize("rows", [16, 64])
def test_attention_backward_rows_option(_attn_children, rows):
    """launch_attn_backward: no attn_bwd_rows setting changes WHICH kernel writes the bijector's partial rows (always
    k_attn_bwd_dx_mfma here, see test_attention_routes); the setting changes which kernels produce the dqkv rows that
    writer reads - the default on these sparse batches is the one-launch k_attn_bwd_edges with 32-row tiles, 64 is the same
    kernel with 64-row tiles, 16 the two-launch k_attn_bwd_recv_rows / k_attn_bwd_send_rows.  Loss, moments, reconstruction
    and every gradient (the bijectors' included) of every attention case, both paths, under each."""
    path = _attn_children(rows)
    for c in B.ATTN_CASES:
        ref = B.reference(c)
        for fused in (True, False):
            rep = B.Report(f"{B.case_id(c)} {'fused' if fused else 'layered'} attn_bwd_rows={rows}")
            got = B.load_child(path, c, fused)
            B.check_forward_terms(rep, got, ref, c.n, tag="train:")
            B.check_reconstruction(rep, got, B.problem(c)["x"])
            B.check_grads(rep, got, ref, c)
            rep.finish()


# ---- 6. gnf_bn_post_step_f32 past one launch -----------------------------------------------------------------------------
def test_post_step_second_launch():
    """T = 25: 50 bijectors, k_bn_post_step in launches of 48 + 2 (BnPostBatch holds 48 descriptors); bijectors 48 and 49
    (half 1, i = 23 and 24) are the second launch.  gamma entries of EVERY bijector (one of the two, or both: three
    patterns in turn) are set to -0.3 and 0 between
    loss_and_grads and apply_gradients (the two calls tr.step makes) - a non-positive gamma cannot go through the forward
    pass, whose log-det term is log(gamma), in the library or in the oracle.  After the step every gamma must be
    max(gamma_after_adam, 0) + 1e-6, gamma_after_adam from O.adam_step on the gradient the trainer holds (Adam is
    elementwise fp32: the project's rtol 2e-6), and both moving statistics moving * m + batch * (1 - m) elementwise to
    float32 rounding (three roundings of O(1) values: 4e-7 + 4e-7 |ref|); the batch moments and every gradient of the
    step (the fifty bijectors' gamma / beta among them) are held to the oracle's first."""
    from gnf_amd.train import GRevNetTrainer
    c = mp(4, 40, latent=8, k=1, t=25)
    ref, pr = B.reference(c), B.problem(c)
    t, lr = c.t, 1e-2
    net, graph = B.make_net(c, True), B.device_graph(c)
    tr = GRevNetTrainer(net, lr=lr, use_lr_decay=False)
    out = tr.loss_and_grads(graph)
    torch.cuda.synchronize()
    rep = B.Report("post-step T25")
    got = dict(z=out["z_graph"].nodes.cpu().numpy(), loss=float(out["total_loss"]), logdet=float(out["log_det_jacobian"]),
               moments=B._device_moments(net, t))
    got["grads"] = B.flat_grads(tr.named_gradients())
    B.check_forward_terms(rep, got, ref, c.n, tag="train:")
    B.check_grads(rep, got, ref, c)             # (K = 1: no hidden unit, no kink; holds bijectors 48 and 49 of the backward walk)
    rep.finish()
    before, grads = {}, dict(got["grads"])
    for half in range(2):
        for i in range(t):
            bn = net.bns[half][i]
            q = half * t + i                 # (bn.gamma is a view into the trainer's arena; 48: pattern 0, 49: pattern 1)
            if q % 3 != 1:
                bn.gamma[0] = -0.3 if q % 3 == 0 else 0.0
            if q % 3 != 0:
                bn.gamma[1] = 0.0 if q % 3 == 1 else -0.3
            before[half, i] = {k: getattr(bn, k).cpu().numpy().astype(np.float64)
                               for k in ("gamma", "moving_mean", "moving_variance", "batch_mean", "batch_variance")}
    tr.apply_gradients()
    torch.cuda.synchronize()
    m = net.bns[0][0].momentum
    bad = []
    for half in range(2):
        for i in range(t):
            bn, b0, q = net.bns[half][i], before[half, i], half * t + i
            g = grads[f"bn[{half}][{i}].gamma"].astype(np.float64)
            after, _, _ = O.adam_step(b0["gamma"], g, 0 * g, 0 * g, 1, lr, 0.9, 0.9, 1e-8)
            want = np.maximum(after, 0.0) + 1e-6
            err = np.abs(bn.gamma.cpu().numpy() - want)
            if not (err <= 2e-6 * np.abs(want) + 1e-9).all():
                bad.append(f"bijector {q}: gamma {bn.gamma.cpu().numpy()} != {want}")
            for mov, bat in (("moving_mean", "batch_mean"), ("moving_variance", "batch_variance")):
                want = b0[mov] * m + b0[bat] * (1.0 - m)
                err = np.abs(getattr(bn, mov).cpu().numpy() - want)
                if not (err <= 4e-7 + 4e-7 * np.abs(want)).all():
                    bad.append(f"bijector {q}: {mov} {getattr(bn, mov).cpu().numpy()} != {want}")
                # the statistics did move (momentum 0.99 of a 0.3 .. 2-sized gap is far above the bound)
                if not (np.abs(want - b0[mov]) > 1e-5).any():
                    bad.append(f"bijector {q}: {mov} was not expected to move - the test checks nothing")
    assert not bad, "\n".join(bad)
