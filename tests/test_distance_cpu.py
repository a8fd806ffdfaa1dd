"""include/gnf_distance.h - the loss and the two decoders under a distance function given as an argument, and the loss's gradient
with respect to temp and shift - as far as it needs no GPU: the symbols, the workspace size against its documented layout,
every documented error code before any launch, the float64 closed form of the parameter gradient (tests/distance_ref.py)
against central differences of adj_loss_ref.binary_loss, the bound the GPU tests apply checked on a float32 restatement for
every one of their cases, and the Python layer's argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gnf_amd import _abi

import adj_loss_ref as R
import distance_ref as DR

NEW_SYMBOLS = ("gnf_pred_adj_dist_f32", "gnf_adj_edges_count_dist_f32", "gnf_adj_loss_dist_workspace_bytes",
               "gnf_adj_loss_dist_f32")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_distance.h (included by gnf.h), the library's exports and _abi.DISTANCE_SYMBOLS are in step, and the new
    table shares nothing with the others"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_distance.h"$', main, flags=re.M)
    assert main.index('#include "gnf_adj_loss.h"') < main.index('#include "gnf_distance.h"')   # it uses GnfAdjLossSpec
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_distance.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.DISTANCE_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS,
                  _abi.ENCODER_TRAIN_SYMBOLS):
        assert not set(_abi.DISTANCE_SYMBOLS) & set(other)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    assert _abi.ADJ_LOSS_SYMBOLS == ("gnf_adj_loss_workspace_bytes", "gnf_adj_loss_f32")
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    assert C.sizeof(_abi.GnfDistance) == 24 and _abi.GnfDistance.params.offset == 16
    assert C.sizeof(_abi.GnfAdjLossSpec) == 24


def test_workspace_size_is_the_documented_layout():
    lib = _abi.lib()
    old, new = lib.gnf_adj_loss_workspace_bytes, lib.gnf_adj_loss_dist_workspace_bytes
    # gnf_adj_loss_f32's layout | row dtemp, row dshift fp64 [N] | graph dtemp, graph dshift fp64 [B]
    for b, n, cap in ((4, 100, 64), (4, 100, 65), (1, 1, 1), (7, 101, 300), (0, 0, 0), (300, 5, 65536), (3, 0, 10)):
        assert old(b, n, cap) % 8 == 0
        assert new(b, n, cap) == old(b, n, cap) + 2 * n * 8 + 2 * b * 8, (b, n, cap)
    assert new(4, 100, 64) == 2 * 100 * 1 * 8 + 100 * 8 + 2 * 100 * 4 + 2 * 100 * 8 + 2 * 4 * 8
    assert new(-1, 10, 10) == 0 and new(3, -1, 10) == 0 and new(3, 10, -1) == 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _spec(temp=10.0, shift=1.0, by_sqrt=1, soft=0, eps=0.1, tol=0.5):
    return _abi.GnfAdjLossSpec(temp, shift, by_sqrt, soft, eps, tol)


def _dist(temp=3.0, shift=2.0, by_sqrt=1, params=None):
    return _abi.GnfDistance(temp, shift, by_sqrt, params)


def _loss(csr=None, z=P, ld=8, d=8, cap=20, spec=None, dist=None, loss=P, sums=P, fp=P, fn=P, grad=P, ldg=8, scale=1.0,
          gp=P, ws=P, ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    spec = _spec() if spec is None else spec
    dist = _dist() if dist is None else dist
    return _abi.lib().gnf_adj_loss_dist_f32(C.byref(csr), z, ld, d, cap, C.byref(spec), C.byref(dist), loss, sums, fp, fn,
                                            grad, ldg, scale, gp, ws, ws_bytes, None)


def test_loss_validation_without_a_gpu():
    """gnf_adj_loss_f32's checks and codes (tests/test_adj_loss_cpu.py), plus GNF_EINVAL for a null dist; every call here fails
    a check (one that passed them all would launch on these fake pointers)"""
    lib = _abi.lib()
    err = lambda: lib.gnf_last_error().decode()
    args = (P, 8, 8, 20)
    tail = (P, P, P, P, P, 8, 1.0, P, P, 1 << 20, None)
    assert lib.gnf_adj_loss_dist_f32(C.byref(_csr()), *args, C.byref(_spec()), None, *tail) == EINVAL and "dist" in err()
    assert lib.gnf_adj_loss_dist_f32(None, *args, C.byref(_spec()), C.byref(_dist()), *tail) == EINVAL
    assert lib.gnf_adj_loss_dist_f32(C.byref(_csr()), *args, None, C.byref(_dist()), *tail) == EINVAL
    assert _loss(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _loss(csr=_csr(b=0)) == EINVAL
    for name in ("z", "loss", "sums", "fp", "fn", "ws"):
        assert _loss(**{name: None}) == EINVAL, name
    assert _loss(csr=_csr(rowptr=None)) == EINVAL and _loss(csr=_csr(col=None)) == EINVAL
    assert _loss(d=0) == ESHAPE and _loss(d=-3) == ESHAPE and _loss(ld=7) == ESHAPE and "ld" in err()
    assert _loss(ldg=7) == ESHAPE
    assert _loss(csr=_csr(n=-1)) == ESHAPE and _loss(csr=_csr(e=-1)) == ESHAPE and _loss(csr=_csr(b=-1)) == ESHAPE
    assert _loss(cap=-1) == ESHAPE and _loss(cap=65537) == ESHAPE and _loss(cap=0) == ESHAPE
    for eps in (-0.01, 0.51, float("nan")):
        assert _loss(spec=_spec(eps=eps)) == ESHAPE and "label_epsilon" in err()
    assert _loss(spec=_spec(tol=-0.1)) == ESHAPE
    # GNF_EWORKSPACE, the last check: the dist layout is what is asked for, with or without grad_params / device parameters
    need, old = lib.gnf_adj_loss_dist_workspace_bytes(3, 40, 20), lib.gnf_adj_loss_workspace_bytes(3, 40, 20)
    assert need == old + 2 * 40 * 8 + 2 * 3 * 8
    assert _loss(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err() and "gnf_adj_loss_dist_f32" in err()
    assert _loss(ws_bytes=old) == EWORKSPACE
    assert _loss(gp=None, ws_bytes=need - 1) == EWORKSPACE
    assert _loss(dist=_dist(params=P), ws_bytes=need - 1) == EWORKSPACE
    assert _loss(ldg=7, grad=None, ws_bytes=need - 1) == EWORKSPACE   # no gradient: ld_grad is not read


def _pred(dist="default", z=P, ld=8, d=8, n_node=P, b=3, cap=20, out=P, off=P, ws=P, ws_bytes=1 << 20):
    dist = C.byref(_dist()) if dist == "default" else dist
    return _abi.lib().gnf_pred_adj_dist_f32(dist, z, ld, d, n_node, b, cap, out, off, ws, ws_bytes, None)


def _count(dist="default", z=P, ld=8, d=8, n_node=P, b=3, n=40, cap=20, thr=0.5, loops=0, rowptr=P, n_edge=P, total=P, ws=P,
           ws_bytes=1 << 20):
    dist = C.byref(_dist()) if dist == "default" else dist
    return _abi.lib().gnf_adj_edges_count_dist_f32(dist, z, ld, d, n_node, b, n, cap, thr, loops, rowptr, n_edge, total, ws,
                                                   ws_bytes, None)


def test_decoder_validation_without_a_gpu():
    """the codes of gnf_pred_adj_f32 and gnf_adj_edges_count_f32, plus GNF_EINVAL for a null dist"""
    lib = _abi.lib()
    err = lambda: lib.gnf_last_error().decode()
    assert _pred(dist=None) == EINVAL and "dist" in err()
    assert _pred(d=0) == ESHAPE and _pred(ld=7) == ESHAPE and _pred(b=-1) == ESHAPE and _pred(cap=-1) == ESHAPE
    for name in ("z", "n_node", "out", "off", "ws"):
        assert _pred(**{name: None}) == EINVAL, name
    assert _pred(ws_bytes=lib.gnf_pred_adj_workspace_bytes(3) - 1) == EWORKSPACE and "gnf_pred_adj_dist_f32" in err()
    assert _count(dist=None) == EINVAL and "dist" in err()
    assert _count(d=0) == ESHAPE and _count(ld=7) == ESHAPE and _count(b=-1) == ESHAPE and _count(n=-1) == ESHAPE
    assert _count(cap=-1) == ESHAPE and _count(cap=0) == ESHAPE
    assert _count(n=1 << 20, cap=1 << 12) == ESHAPE and "int32" in err()
    for name in ("z", "n_node", "rowptr", "n_edge", "total", "ws"):
        assert _count(**{name: None}) == EINVAL, name
    assert _count(ws_bytes=lib.gnf_adj_edges_workspace_bytes(3, 40, 20) - 1) == EWORKSPACE
    assert "gnf_adj_edges_count_dist_f32" in err()


# ---- the reference alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("dist", DR.DISTS, ids=lambda t: f"t{t[0]:g}_s{t[1]:g}_{'scaled' if t[2] else 'unscaled'}")
def test_closed_form_equals_central_differences(dist, soft):
    d = 7
    seed, z, (_, s, r) = R.pick_seed(R.SIZES, d, dist)
    assert seed is not None
    z = z.astype(np.float64)
    got_t, got_s = DR.param_grads(z, R.SIZES, s, r, dist, soft)
    ref = R.binary_loss(z, R.SIZES, s, r, dist, soft)
    live = sum(int((b["off"] & ~b["clipped"]).sum()) for b in ref["blocks"])
    clipped = sum(int(b["clipped"].sum()) for b in ref["blocks"])
    assert live > 1000 and clipped > 100                             # both branches of the rule see many pairs
    # the margin (2 delta >= 2^-15 in the logit) keeps a step of 1e-6 in temp or shift (at most 2e-5 in the logit) off the kinks
    h = 1e-6
    temp, shift, by_sqrt = dist
    loss = lambda t, sh: R.binary_loss(z, R.SIZES, s, r, (t, sh, by_sqrt), soft)["sum_loss"]
    fd_t = (loss(temp + h, shift) - loss(temp - h, shift)) / (2.0 * h)
    fd_s = (loss(temp, shift + h) - loss(temp, shift - h)) / (2.0 * h)
    print(f"{dist} soft={soft}: dtemp {got_t:.10g} fd {fd_t:.10g}, dshift {got_s:.10g} fd {fd_s:.10g}, {live} live pairs")
    # roundoff of a loss below 1e5 over 2e-6 is below 1e-5; truncation h^2 f''' far below that
    assert abs(fd_t - got_t) <= 1e-5 * max(abs(got_t), 1.0) and abs(fd_s - got_s) <= 1e-5 * max(abs(got_s), 1.0)
    assert abs(got_t) > 1.0 and abs(got_s) > 1.0


# ---- the GPU tests' bound, on a float32 restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("c", DR.GRAD_CASES, ids=DR.case_id)
def test_a_float32_restatement_keeps_the_gpu_tests_bound(c):
    d, dist, soft = c
    seed, z, graph = DR.grad_case(*c)
    assert seed is not None, f"{DR.case_id(c)}: no seed in range(16) keeps every pair 2 delta from the kinks"
    _, s, r = graph
    ref = DR.param_grads(z, R.SIZES, s, r, dist, soft)
    got = DR.param_grads_f32(z, R.SIZES, s, r, dist, soft)
    bound = DR.param_grad_bounds(z, R.SIZES, s, r, dist, soft)
    ratios = [abs(g - w) / b if b > 0 else (0.0 if g == w else np.inf) for g, w, b in zip(got, ref, bound)]
    print(f"{DR.case_id(c)}: seed {seed}, dtemp {ref[0]:.8g} dshift {ref[1]:.8g}, float32 error / bound {ratios[0]:.3g} "
          f"{ratios[1]:.3g}")
    assert abs(got[0] - ref[0]) <= bound[0] and abs(got[1] - ref[1]) <= bound[1]


# ---- Python layer ----------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd import adj_loss, encoder, flow
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    from gnf_amd.train import EncoderTrainer
    assert gnf_amd.TunedSigmoidL2 is adj_loss.TunedSigmoidL2
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    tuned = adj_loss.TunedSigmoidL2(3, 2)
    assert tuned.params is None and tuned.values() == (3.0, 2.0) and adj_loss.TunedSigmoidL2().values() == (10.0, 1.0)
    for tok in (scaled_hacky_sigmoid_l2, adj_loss.hacky_sigmoid_l2, adj_loss.sigmoid_l2(3.0, 2.0)):
        with pytest.raises(ValueError):                              # a fixed token's parameters have no gradient
            adj_loss.binary_loss(g, g, distance_fn=tok, grad_params=True)
    tokens = (scaled_hacky_sigmoid_l2, adj_loss.hacky_sigmoid_l2, adj_loss.sigmoid_l2(3.0, 2.0), tuned)
    for tok in tokens:                                               # CPU tensors: no fallback, for any token
        with pytest.raises(_abi.GnfError):
            adj_loss.binary_loss(g, g, distance_fn=tok)
        with pytest.raises(_abi.GnfError):
            flow.pred_adj(g, distance_fn=tok)
        with pytest.raises(_abi.GnfError):
            flow.decode_graphs(g, distance_fn=tok)
    with pytest.raises(_abi.GnfError):
        adj_loss.binary_loss(g, g, distance_fn=tuned, grad_params=True)
    assert tuned.params is None                                      # nothing was created on the way
    with pytest.raises(_abi.GnfError):
        tuned.bind(torch.zeros(2))
    for fn in (flow.pred_adj, flow.decode_graphs, lambda *a, **k: adj_loss.binary_loss(g, *a, **k)):
        with pytest.raises(NotImplementedError):
            fn(g, distance_fn=lambda nodes: nodes)
        with pytest.raises(NotImplementedError):
            fn(g, distance_fn=adj_loss.sigmoid_l2)                   # the class, not a token made from it
    # the trainer: tune_sigmoid trains sigmoid_l2's parameters and nothing else's (run_gnn.py:148-153)
    enc = encoder.make_encoder(dict(node_dim=4, latent=8, K=2, activation="leaky_relu", num_timesteps=1, agg="mean",
                                    combine="agg", epsilon=1.0))
    for tok in (None, scaled_hacky_sigmoid_l2, adj_loss.hacky_sigmoid_l2):
        with pytest.raises(ValueError):
            EncoderTrainer(enc, distance_fn=tok, tune_sigmoid=True)
    tr = EncoderTrainer(enc, distance_fn=adj_loss.sigmoid_l2(3.0, 2.0), tune_sigmoid=True)
    assert isinstance(tr.distance_fn, adj_loss.TunedSigmoidL2) and tr.distance_fn.values() == (3.0, 2.0)
    assert EncoderTrainer(enc, distance_fn=tuned, tune_sigmoid=True).distance_fn is tuned
    assert EncoderTrainer(enc).tune_sigmoid is False
    # save_encoder's "distance" entry and distance_of
    assert encoder.distance_of({}) is scaled_hacky_sigmoid_l2
    assert encoder.distance_entry(adj_loss.hacky_sigmoid_l2) == {"kind": "hacky_sigmoid_l2", "temp": 10.0, "shift": 1.0}
    assert encoder.distance_of({"distance": encoder.distance_entry(adj_loss.hacky_sigmoid_l2)}) is adj_loss.hacky_sigmoid_l2
    assert encoder.distance_of({"distance": encoder.distance_entry(scaled_hacky_sigmoid_l2)}) is scaled_hacky_sigmoid_l2
    back = encoder.distance_of({"distance": encoder.distance_entry(tuned)})
    assert isinstance(back, adj_loss.sigmoid_l2) and (back.temp, back.shift) == (3.0, 2.0)
    with pytest.raises(ValueError):
        encoder.distance_of({"distance": {"kind": "exp_l2", "temp": 1.0, "shift": 1.0}})
