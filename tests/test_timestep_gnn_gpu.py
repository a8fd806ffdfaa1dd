"""gnf_amd.gnn.TimestepGNN / gnf_timestep_gnn_f32 on the device (include/gnf_timestep_gnn.h), and what consumes it
(gnf_amd.encoder).

Bitwise where the header promises bits: without norms the call is T chained gnf_gnn_apply_f32 calls (plus one fp32 add per
element with the residual); two calls, and a captured call replayed, give the same bits; the moving statistics advance by
exactly one separately-rounded fp32 update per training call.  Everything else is compared with the float64 restatement
(tests/timestep_gnn_ref.py) under the rule of tests/batch_norm_routes.py: per case the larger of that module's own bound
(z: 5e-4 max(1, |ref|max); batch mean 3e-5; batch variance 3e-5 (1 + |ref|)) and 4 x what the float32 restatement itself
differs from float64 by on the same case.  The inputs of every whole-module case satisfy the restatement's seed condition
(no hidden unit within 4 float32 deviations of its activation's kink: tests/test_timestep_gnn_cpu.py), so every element is
compared.  Every figure is printed before it is asserted (pytest -s).

Measured on the MI355X, worst ratio (device deviation / bound) over the quantities of a case; no bound was changed.
  norm stage (y, batch and moving moments; BN, LN, BN + LN), rows n, columns D =     1     2     6    64   100   130   257
    n = 1                                    0.002 0.043 0.151 0.203 0.068 0.154 0.571
    n = 17                                   0.000 0.092 0.065 0.060 0.042 0.075 0.042
    n = 32                                   0.001 0.119 0.087 0.066 0.048 0.111 0.095
    n = 33                                   0.004 0.082 0.045 0.069 0.116 0.043 0.077
    n = 513                                  0.001 0.439 0.091 0.117 0.116 0.070 0.043
  (largest: y of BN at n = 1, D = 257 - x * inv and mean * inv near 4.7e3 cancel in fp32, as the formula has it - and y of
  BN + LN at n = 513, D = 2 - two features, one of them constant: the float32 restatement itself is off by 1.8e-3 there)
  mode training=False local=False: 0.000
  mode training=False local=True: 0.002
  mode training=True local=False: 0.002
  mode training=True local=True: 0.002
  avg_D6_K2_T3_bn_res: 0.002
  avg_D100_K3_T3_bn_ln_shared: 0.003
  avg_D100_K2_T3_ln_res: 0.001
  sumcat_D100_K2_T3_bn_shared: 0.002
  sumcat_D6_K3_T3_bn_ln_res: 0.002
  sumcat_D6_K2_T3_ln_shared: 0.000
  dm_D6_K3_T3_bn_res_shared: 0.002
  dm_D100_K2_T3_bn_ln_res: 0.003
  dm_D100_K3_T3_ln: 0.002
  graph_D100_K3_T3_bn: 0.001
  graph_D6_K2_T3_bn_ln_shared: 0.002
  graph_D6_K3_T3_ln_res_shared: 0.000
  strided sumcat_D6_K3_T3_bn_ln_res: 0.001
  strided dm_D100_K2_T3_bn_ln_res: 0.001
  evaluate avg_D6_K2_T3_bn_res: 0.000
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from gnf_amd import _abi, encoder, gnn
from gnf_amd.graphs import csr_desc, csr_of
from helpers import GuardBanded, graph_from_arrays

import timestep_gnn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _graph(batch, x):
    nn, ne, s, r = batch
    return graph_from_arrays(nn, ne, s, r, x, DEV)


def _encoder(c, params=None, **over):
    enc = encoder.make_encoder(dict(R.family_hp(c), **over))
    return enc.set_params(R.make_params(c) if params is None else params)


class _Report:
    def __init__(self, title):
        self.title, self.bad, self.worst = title, [], 0.0

    def add(self, name, got, ref64, ref32, project):
        err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
        dev = float(np.abs(ref32 - ref64).max())
        bound = max(project, 4.0 * dev)
        self.worst = max(self.worst, err / bound)
        print(f"[timestep-gnn] {self.title} {name}: err {err:.3e} bound {bound:.3e} (project {project:.3e}, float32 restatement "
              f"off by {dev:.3e}) ratio {err / bound:.3f}")
        if not err <= bound:
            self.bad.append(f"{name}: err {err:.3e} > {bound:.3e}")

    def z(self, name, got, ref64, ref32):
        self.add(name, got, ref64, ref32, 5e-4 * max(1.0, float(np.abs(ref64).max())))

    def mean(self, name, got, ref64, ref32):
        self.add(name, got, ref64, ref32, 3e-5)

    def var(self, name, got, ref64, ref32):
        scale = 1.0 + np.abs(ref64)
        self.add(name, np.asarray(got, np.float64) / scale, ref64 / scale, ref32 / scale, 3e-5)
        if not (np.asarray(got) >= 0.0).all():
            self.bad.append(f"{name}: negative variance")

    def finish(self):
        print(f"[timestep-gnn] {self.title}: worst ratio {self.worst:.3f}")
        assert not self.bad, self.title + "\n" + "\n".join(self.bad)


# ---- bit identity with chained gnf_gnn_apply_f32 calls -------------------------------------------------------------------------
@pytest.mark.parametrize("sharing", [False, True], ids=["own_nets", "shared"])
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("family", ["avg", "dm", "graph"])
def test_without_norms_the_call_is_chained_module_calls_bit_for_bit(family, t, sharing):
    c = R.Case(family, 6 if family != "dm" else 100, 32, 2, t, False, False, False, sharing)
    batch, x = R.ring_chord_batch(R.SIZES), R.module_inputs(c, 0)
    graph = _graph(batch, x)
    enc = _encoder(c)
    out = enc(graph, True).nodes
    chain = graph
    for i in range(t):
        chain = enc.gnns[0 if sharing else i](chain)              # gnf_gnn_apply_f32
    torch.cuda.synchronize()
    assert torch.equal(out, chain.nodes) and torch.equal(graph.nodes, torch.as_tensor(x).to(DEV))
    assert torch.isfinite(out).all() and float(out.abs().max()) > 1e-3 and enc.last_batch_moments is None
    enc.residual = True
    res = enc(graph, False).nodes
    assert torch.equal(res, chain.nodes + graph.nodes)              # one fp32 add per element
    if t == 3 and not sharing:                                      # the nets are taken in order
        assert not torch.equal(enc.gnns[2](enc.gnns[0](enc.gnns[1](graph))).nodes, chain.nodes)


# ---- the norm stage alone --------------------------------------------------------------------------------------------------
def _norm_encoder(d, bn, ln, rng):
    mk = partial(gnn.sum_then_mlp_gnn, partial(gnn.make_mlp_model, 8, d, 1, gnn.relu), 1.0)
    enc = gnn.TimestepGNN(mk, 1, use_batch_norm=bn, residual=False, use_layer_norm=ln)
    p = {"nets": [R.identity_net(d)]}
    if bn:
        p["bn"] = R.make_bn_params(rng, d, 1)
    if ln:
        p["ln"] = R.make_ln_params(rng, d, 1)
    return enc.set_params(p), p


@pytest.mark.parametrize("d", R.NORM_WIDTHS)
@pytest.mark.parametrize("sizes", list(R.NORM_SIZES), ids=list(R.NORM_SIZES))
def test_norm_stage_against_float64(sizes, d):
    sizes = R.NORM_SIZES[sizes]
    n = sum(sizes)
    x = R.norm_inputs(n, d)
    graph = _graph(R.edgeless_batch(sizes), x)
    # the rest of the test stands on this: on an edgeless batch sum_then_mlp (eps = 1) with W = I, b = 0 returns its input
    ident, _ = _norm_encoder(d, False, False, None)
    assert torch.equal(ident.gnns[0](graph).nodes, graph.nodes) and torch.equal(ident(graph, True).nodes, graph.nodes)
    rep = _Report(f"norm n={n} D={d}")
    for bn, ln in ((True, False), (False, True), (True, True)):
        tag = ("bn" if bn else "") + ("+" if bn and ln else "") + ("ln" if ln else "")
        enc, p = _norm_encoder(d, bn, ln, np.random.default_rng(100 * d + n))
        got = enc(graph, True).nodes.cpu().numpy()
        r64, r32 = (R.norm_only(x, p["bn"][0] if bn else None, p["ln"][0] if ln else None, dt) for dt in (np.float64, np.float32))
        rep.z(tag + " y", got, r64["y"], r32["y"])
        if bn:
            (bm, bv), b = enc.last_batch_moments[0], enc.bns[0]
            rep.mean(tag + " batch_mean", bm.cpu().numpy(), r64["mean"], r32["mean"])
            rep.var(tag + " batch_variance", bv.cpu().numpy(), r64["var"], r32["var"])
            rep.mean(tag + " moving_mean", b.moving_mean.cpu().numpy(), r64["moving_mean"], r32["moving_mean"])
            rep.var(tag + " moving_variance", b.moving_variance.cpu().numpy(), r64["moving_variance"], r32["moving_variance"])
            assert float(bv[0]) == 0.0 and float(bm[0]) == 0.75     # the constant column: variance exactly 0 (n = 1: all)
    assert torch.equal(graph.nodes, torch.as_tensor(x).to(DEV))
    rep.finish()


# ---- the four (is_training, test_local_stats) modes ------------------------------------------------------------------------
@pytest.mark.parametrize("training,local", [(False, False), (False, True), (True, False), (True, True)])
def test_modes_pick_the_statistics_and_only_training_updates_them(training, local):
    c = R.MODULE_CASES[0]
    seed, x, r64, r32 = R.pick_seed(c, training, local)
    assert seed is not None
    p = R.make_params(c)
    enc = _encoder(c, p, test_local_stats=local)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    for _ in range(3):
        out = enc(graph, training).nodes
    rep = _Report(f"mode training={training} local={local}")
    rep.z("out", out.cpu().numpy(), r64["out"], r32["out"])
    # the other statistics give another result, by far more than any bound: the comparison above tells the modes apart
    other = R.run_case(c, x, np.float64, not (training or local), False, p)["out"]
    assert np.abs(other - r64["out"]).max() > 100 * R.z_bound(r64["out"], r32["out"])
    assert (enc.last_batch_moments is None) == (not training and not local)
    cur64, cur32 = p, p
    for _ in range(3):      # the restatement's moving statistics after three calls
        step64, step32 = R.run_case(c, x, np.float64, training, local, cur64), R.run_case(c, x, np.float32, training, local, cur32)
        cur64, cur32 = (dict(q, bn=[dict(e, moving_mean=mm, moving_variance=mv) for e, (mm, mv) in zip(q["bn"], res["moving"])])
                        for q, res in ((cur64, step64), (cur32, step32)))
    for i, bn in enumerate(enc.bns):
        mm, mv = bn.moving_mean.cpu().numpy(), bn.moving_variance.cpu().numpy()
        if training:
            rep.mean(f"moving_mean[{i}]", mm, cur64["bn"][i]["moving_mean"], cur32["bn"][i]["moving_mean"])
            rep.var(f"moving_variance[{i}]", mv, cur64["bn"][i]["moving_variance"], cur32["bn"][i]["moving_variance"])
            assert not np.array_equal(mm, p["bn"][i]["moving_mean"]) and not np.array_equal(mv, p["bn"][i]["moving_variance"])
        else:
            assert np.array_equal(mm, p["bn"][i]["moving_mean"]) and np.array_equal(mv, p["bn"][i]["moving_variance"])
        if training or local:
            bm, bv = (t.cpu().numpy() for t in enc.last_batch_moments[i])
            rep.mean(f"batch_mean[{i}]", bm, r64["moments"][i][0], r32["moments"][i][0])
            rep.var(f"batch_variance[{i}]", bv, r64["moments"][i][1], r32["moments"][i][1])
    rep.finish()


# ---- the whole module --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.MODULE_CASES, ids=R.case_id)
def test_module_against_float64(c):
    seed, x, r64, r32 = R.pick_seed(c)
    assert seed is not None
    enc = _encoder(c)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    out = enc(graph, True).nodes.cpu().numpy()
    rep = _Report(R.case_id(c))
    rep.z("out", out, r64["out"], r32["out"])
    for i in range(c.t if c.bn else 0):
        bm, bv = (t.cpu().numpy() for t in enc.last_batch_moments[i])
        rep.mean(f"batch_mean[{i}]", bm, r64["moments"][i][0], r32["moments"][i][0])
        rep.var(f"batch_variance[{i}]", bv, r64["moments"][i][1], r32["moments"][i][1])
        rep.mean(f"moving_mean[{i}]", enc.bns[i].moving_mean.cpu().numpy(), r64["moving"][i][0], r32["moving"][i][0])
        rep.var(f"moving_variance[{i}]", enc.bns[i].moving_variance.cpu().numpy(), r64["moving"][i][1], r32["moving"][i][1])
    assert torch.equal(graph.nodes, torch.as_tensor(x).to(DEV))
    rep.finish()


# ---- strides -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [R.MODULE_CASES[4], R.MODULE_CASES[7]], ids=R.case_id)   # sumcat D 6 and dm_attn D 100: BN + LN + residual
def test_strided_x_and_out_leave_guard_bands_and_x_untouched(c):
    seed, x, r64, r32 = R.pick_seed(c)
    enc = _encoder(c)
    n, d = x.shape
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    xin = GuardBanded(n, d, d + 9, c0=3, device=DEV, fill=x)       # ldx > D, the window's base off 16-byte alignment
    out = GuardBanded(n, d, d + 5, c0=1, device=DEV)
    before = xin.bits.clone()
    lib = _abi.lib()
    desc, keep = enc._desc(d, torch.device(DEV), True)
    csr = csr_desc(graph, csr_of(graph), False)
    ws_bytes = lib.gnf_timestep_gnn_workspace_bytes(n, d, C.byref(desc))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _abi.check(lib.gnf_timestep_gnn_f32(C.byref(csr), C.byref(desc), xin.ptr(), xin.ld, out.ptr(), out.ld, d, _abi.ptr(ws), ws_bytes,
                                        _abi.stream_ptr(torch.device(DEV))), "gnf_timestep_gnn_f32")
    torch.cuda.synchronize()
    out.check_guard()
    assert torch.equal(xin.bits, before)                            # x and its guard bands: bitwise untouched
    rep = _Report("strided " + R.case_id(c))
    rep.z("out", out.numpy(), r64["out"], r32["out"])
    rep.finish()
    # overlapping x / out (out starts inside the last row of x) is refused before any launch
    rc = lib.gnf_timestep_gnn_f32(C.byref(csr), C.byref(desc), xin.ptr(), xin.ld, C.c_void_p(xin.ptr().value + 4 * xin.ld * (n - 1)),
                                  xin.ld, d, _abi.ptr(ws), ws_bytes, _abi.stream_ptr(torch.device(DEV)))
    assert rc == -1 and "overlap" in lib.gnf_last_error().decode()
    assert torch.equal(xin.bits, before)


# ---- reproducibility and capture ---------------------------------------------------------------------------------------------
def _f32_update(moving, batch):
    """one moving-average update in separately rounded fp32 operations, as the header states it"""
    omd = np.float32(1.0) - np.float32(R.BN_DECAY)
    return (moving - ((moving - batch).astype(np.float32) * omd).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("c", [R.MODULE_CASES[1], R.MODULE_CASES[10]], ids=R.case_id)   # avg D 100 and graph-scope D 6: BN + LN, shared
def test_two_calls_and_a_replayed_capture_give_the_same_bits(c):
    x = R.module_inputs(c, 0)
    p = R.make_params(c)
    enc = _encoder(c, p)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    e1 = enc(graph, True).nodes.clone()
    e2 = enc(graph, True).nodes.clone()
    batch = [(m.cpu().numpy().copy(), v.cpu().numpy().copy()) for m, v in enc.last_batch_moments]
    ev = enc(graph, False).nodes.clone()                             # (the moving statistics normalise: other rows, no update)
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and not torch.equal(e1, ev) and enc.last_batch_moments is None
    want = [(pb["moving_mean"], pb["moving_variance"]) for pb in p["bn"]]
    for _ in range(2):                                               # two training calls so far: two updates, exactly
        want = [(_f32_update(mm, bm), _f32_update(mv, bv)) for (mm, mv), (bm, bv) in zip(want, batch)]
    for b, (mm, mv) in zip(enc.bns, want):
        assert np.array_equal(b.moving_mean.cpu().numpy(), mm) and np.array_equal(b.moving_variance.cpu().numpy(), mv)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        out_c = enc(graph, True).nodes
    torch.cuda.synchronize()
    for b, (mm, mv) in zip(enc.bns, want):                           # capturing runs nothing
        assert np.array_equal(b.moving_mean.cpu().numpy(), mm)
    for k in range(2):
        out_c.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_c, e1), k
        want = [(_f32_update(mm, bm), _f32_update(mv, bv)) for (mm, mv), (bm, bv) in zip(want, batch)]
        for b, (mm, mv) in zip(enc.bns, want):                       # ... and a replay advances them exactly once
            assert np.array_equal(b.moving_mean.cpu().numpy(), mm) and np.array_equal(b.moving_variance.cpu().numpy(), mv), k


# ---- what consumes the encoder -----------------------------------------------------------------------------------------------
def test_evaluate_is_binary_loss_on_the_encoders_output():
    from gnf_amd import adj_loss
    c = R.MODULE_CASES[0]
    seed, x, ref64, ref32 = R.pick_seed(c, False, False)            # evaluation: the moving statistics normalise
    assert seed is not None
    enc = _encoder(c)
    graph = _graph(R.ring_chord_batch(R.SIZES), x)
    ev = encoder.evaluate(enc, graph, use_soft_labels=True)
    out = enc(graph, False)
    res = adj_loss.binary_loss(out, graph, use_soft_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(ev["gnn_output"].nodes, out.nodes)
    assert float(ev["sum_loss"]) == float(res["sum_loss"]) > 0.0 and float(ev["mean_loss"]) == float(res["mean_loss"])
    fp, fn = int(res["false_positive_pairs"].sum()), int(res["false_negative_pairs"].sum())
    assert float(ev["false_positive_edges"]) == fp / 2 and float(ev["false_negative_edges"]) == fn / 2
    assert float(ev["total_incorrect_edges"]) == (fp + fn) / 2 > 0
    assert float(ev["incorrect_edges_per_node"]) == (fp + fn) / 2 / 69
    assert torch.equal(ev["incorrect_edges_per_graph"], adj_loss.incorrect_edges_per_graph(res))
    # is_training=False: evaluation used the moving statistics (the parameters' own) and left them alone
    assert enc.last_batch_moments is None
    p = R.make_params(c)
    assert all(np.array_equal(b.moving_mean.cpu().numpy(), q["moving_mean"]) for b, q in zip(enc.bns, p["bn"]))
    rep = _Report("evaluate " + R.case_id(c))
    rep.z("gnn_output", out.nodes.cpu().numpy(), ref64["out"], ref32["out"])
    rep.finish()


class _Batches:
    """a dataset stand-in: get_next_train_batch draws ring + chord batches with fresh features and remembers them"""

    def __init__(self, d):
        self.rng, self.d, self.seen = np.random.default_rng(5), d, []

    def get_next_train_batch(self, batch_size, device=None):
        assert batch_size == 5
        x = self.rng.standard_normal((69, self.d)).astype(np.float32)
        g = graph_from_arrays(*R.ring_chord_batch(R.SIZES), x, device)
        self.seen.append(g)
        return g


def test_chunks_round_trip_bit_for_bit(tmp_path):
    from gnf_amd.datasets import GrevnetDatasetFixed, GrevnetDatasetVariable
    c = R.MODULE_CASES[0]
    enc = _encoder(c)
    ds = _Batches(c.d)
    # 3 batches of 5 graphs for 12 examples; 69 rows x 6 floats = 1656 bytes per batch: a chunk closes after two batches
    paths = encoder.write_embedding_chunks(enc, ds, str(tmp_path), 12, 5, device=DEV, chunk_bytes=2000)
    assert len(paths) == 2 and len(ds.seen) == 3 and enc.last_batch_moments is None
    want = [enc(g, False).nodes.cpu().numpy() for g in ds.seen]
    fixed = GrevnetDatasetFixed(str(tmp_path), 5, sort_files=True)
    for k in range(3):
        emb, n_node = fixed.train_batch()
        assert emb.dtype == np.float32 and np.array_equal(emb, want[k]) and list(n_node) == R.SIZES
    with pytest.raises(IndexError):
        fixed.train_batch()
    var = GrevnetDatasetVariable(str(tmp_path), 70, sort_files=True)
    emb, n_node = var.train_batch()
    assert np.array_equal(emb, want[0]) and list(n_node) == R.SIZES


def test_the_data_example_makes_its_chunks_from_an_encoder_file(tmp_path):
    """examples/train_grevnet_with_data.py --make_chunks --encoder_params FILE: the chunks come from the saved encoder's
    forward pass over --dataset, and the flow trains and samples at the encoder's node width (tiny flags: two iterations)"""
    import os
    import subprocess
    import sys
    c = R.MODULE_CASES[0]
    hp = R.family_hp(c)
    path = str(tmp_path / "encoder.npz")
    encoder.save_encoder(path, hp, _encoder(c))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "examples", "train_grevnet_with_data.py"), "--make_chunks",
                          "--encoder_params", path, "--dataset", "graph_rnn_community_small", "--attn_type", "avg_then_mlp",
                          "--latent_dim", "16", "--num_layers", "2", "--num_coupling_layers", "2", "--train_batch_size", "4",
                          "--num_train_iters", "2", "--log_every_n_steps", "1", "--sample_size", "2", "--clip_gradient_by_norm"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "embedding chunks from the encoder" in run.stdout and "iteration     2" in run.stdout
    assert f"batch nodes" in run.stdout and "sampled graph 1" in run.stdout
