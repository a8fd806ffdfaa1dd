"""gnf_amd.gnn.TimestepGNN / gnf_timestep_gnn_f32: everything that needs no GPU - the restatement the GPU tests compare against
(tests/timestep_gnn_ref.py) against closed forms, the seed condition on every case the GPU tests use, the symbols and struct
sizes, the host-side workspace size, the argument validation before any launch and the Python layer's errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import timestep_gnn_ref as R

NEW_SYMBOLS = ("gnf_timestep_gnn_workspace_bytes", "gnf_timestep_gnn_f32")
P = 0x1000   # a non-null pointer that validation never dereferences
OK, EINVAL, ESHAPE, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5


# ---- the restatement against closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["avg", "sumcat", "dm", "graph"])
def test_one_timestep_without_norms_is_one_module_call(family):
    c = R.Case(family, 6, 32, 2, 1, False, False, False, False)
    batch, p, x = R.ring_chord_batch(R.SIZES), R.make_params(c), R.module_inputs(c, 0)
    got = R.forward(batch, x, p, 1, np.float64, family, residual=False)
    o = R.GA.GraphAttnGather(batch[2], batch[3], batch[0], **R.family_kw(family))
    want = o.gnn(o.to_t(x), o.prep_params({"nets": p["nets"]})["nets"][0]).numpy()
    assert np.array_equal(got["out"], want) and got["moments"] == [] and sorted(got["pre"]) == [(0, 0)]
    res = R.forward(batch, x, p, 1, np.float64, family, residual=True)
    assert np.array_equal(res["out"], want + x.astype(np.float64))


def test_batch_norm_of_a_constant_column_and_of_one_row():
    rng = np.random.default_rng(0)
    bn = R.make_bn_params(rng, 3, 1)[0]
    x = rng.standard_normal((9, 3))
    x[:, 1] = 0.75
    out = R.norm_only(x, bn, None, np.float64)
    assert out["var"][1] == 0.0 and out["mean"][1] == 0.75
    np.testing.assert_allclose(out["y"][:, 1], np.float64(bn["beta"][1]), rtol=0, atol=1e-13)    # (x - mean) inv = 0
    want = (x - x.mean(0)) / np.sqrt(x.var(0) + R.BN_EPS) * bn["gamma"].astype(np.float64) + bn["beta"].astype(np.float64)
    np.testing.assert_allclose(out["y"], want, rtol=0, atol=1e-12)
    one = R.norm_only(x[:1], bn, None, np.float64)                                            # n = 1: every variance 0
    assert not one["var"].any() and np.array_equal(one["mean"], x[0])
    np.testing.assert_allclose(one["y"][0], bn["beta"].astype(np.float64), rtol=0, atol=1e-12)
    # evaluation without test_local_stats: the moving statistics, whatever the batch holds
    ev = R.norm_only(x, bn, None, np.float64, is_training=False)
    mm, mv = bn["moving_mean"].astype(np.float64), bn["moving_variance"].astype(np.float64)
    np.testing.assert_allclose(ev["y"], (x - mm) / np.sqrt(mv + R.BN_EPS) * bn["gamma"] + bn["beta"], rtol=0, atol=1e-12)
    assert "moving_mean" not in ev and np.array_equal(R.norm_only(x, bn, None, np.float64, False, True)["y"], out["y"])


def test_moving_update_after_k_steps_is_geometric():
    m0, b = torch.tensor([0.0, 1.0, -3.0], dtype=torch.float64), torch.tensor([2.0, 0.25, 5.0], dtype=torch.float64)
    m = m0
    for k in range(1, 6):
        m = R.moving_update(m, b)
        np.testing.assert_allclose(m.numpy(), (b + (m0 - b) * R.BN_DECAY ** k).numpy(), rtol=1e-13, atol=0)
    # through forward(): T batch norms, each updated once per training call, none in evaluation
    c = R.Case("avg", 6, 32, 2, 3, True, False, True, False)
    p, x = R.make_params(c), R.module_inputs(c, 0)
    cur = p
    for _ in range(3):
        res = R.run_case(c, x, np.float64, is_training=True, params=cur)
        cur = dict(cur, bn=[dict(b_, moving_mean=mm, moving_variance=mv) for b_, (mm, mv) in zip(cur["bn"], res["moving"])])
    for i in range(3):
        mean, var = res["moments"][i]
        for key, batch in (("moving_mean", mean), ("moving_variance", var)):
            want = batch + (p["bn"][i][key].astype(np.float64) - batch) * R.BN_DECAY ** 3
            np.testing.assert_allclose(cur["bn"][i][key], want, rtol=1e-12, atol=1e-15)
    ev = R.run_case(c, x, np.float64, is_training=False, params=p)
    assert ev["moments"] == [None] * 3
    assert all(np.array_equal(mm, p["bn"][i]["moving_mean"]) for i, (mm, _) in enumerate(ev["moving"]))


def test_layer_norm_of_a_row_with_known_moments():
    ln = {"gamma": np.array([1.0, 2.0, 0.5, 1.0]), "beta": np.array([0.0, 1.0, -1.0, 0.25])}
    row = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 5.0, 5.0, 5.0]])         # mean 2.5, biased variance 1.25; a constant row
    y = R.norm_only(row, None, ln, np.float64)["y"]
    np.testing.assert_allclose(y[0], (row[0] - 2.5) / np.sqrt(1.25 + 1e-5) * ln["gamma"] + ln["beta"], rtol=1e-14)
    np.testing.assert_allclose(y[1], ln["beta"], rtol=0, atol=1e-12)
    both = R.norm_only(np.random.default_rng(1).standard_normal((7, 4)), R.make_bn_params(np.random.default_rng(2), 4, 1)[0], ln,
                       np.float64)["y"]
    g, b = ln["gamma"], ln["beta"]
    np.testing.assert_allclose(((both - b) / g).mean(1), 0.0, atol=1e-12)    # BN then LN: rows end up standardised


# ---- the seed condition on every case the GPU tests use ------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.MODULE_CASES, ids=R.case_id)
def test_a_seed_with_margin_exists_for_every_module_case(c):
    seed, x, r64, r32 = R.pick_seed(c)
    assert seed is not None, f"{R.case_id(c)}: no seed in range(16) keeps every hidden unit 4 deviations from its kink"
    assert x.dtype == np.float32 and x.shape == (69, c.d) and r64["out"].shape == (69, c.d)
    assert sorted(r64["pre"]) == [(i, j) for i in range(c.t) for j in range(c.k - 1)]
    units = sum(v.size for v in r64["pre"].values())
    neg = sum(int((v < 0).sum()) for v in r64["pre"].values()) / units
    print(f"{R.case_id(c)}: seed {seed}, {units} hidden units, {100 * neg:.0f} % negative, float32 restatement off by "
          f"{np.abs(r32['out'] - r64['out']).max():.2e}, bound {R.z_bound(r64['out'], r32['out']):.2e}")
    assert 0.1 < neg < 0.9 and np.isfinite(r64["out"]).all() and np.abs(r64["out"]).max() < 100.0
    assert len(r64["moments"]) == (c.t if c.bn else 0)


def test_a_seed_with_margin_exists_for_the_mode_cases():
    c = R.MODULE_CASES[0]
    for training, local in ((False, False), (False, True), (True, True)):
        assert R.pick_seed(c, training, local)[0] is not None, (training, local)


# ---- ABI without a device ----------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_timestep_gnn.h (included by gnf.h), the library's exports and _abi.ENCODER_SYMBOLS are in step"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_timestep_gnn.h"$', main, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_timestep_gnn.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.ENCODER_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS):
        assert not set(_abi.ENCODER_SYMBOLS) & set(other)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    assert C.sizeof(_abi.GnfSntBatchNorm) == 48 and C.sizeof(_abi.GnfRowNorm) == 16 and C.sizeof(_abi.GnfTimestepGnn) == 80


def _mlp(dims, attn=None):
    m = _abi.GnfMlp()
    m.num_layers = len(dims) - 1
    for j, d in enumerate(dims):
        m.dims[j] = d
    for j in range(len(dims) - 1):
        m.W[j] = P
        m.b[j] = P
    if attn is not None:
        m.attn = C.pointer(attn)
    return m


class _Enc:
    """a GnfTimestepGnn on fake pointers, with everything it points to kept alive"""

    def __init__(self, t=3, d=8, dims=None, sharing=0, bn=True, ln=True, residual=1, training=1, local=0, eps=1e-3, decay=0.999,
                 combine=0, nets=None, bn_null=(), ln_null=()):
        dims = [d, 16, d] if dims is None else dims
        n_nets = 1 if sharing else max(t, 1)
        self.nets = (_abi.GnfMlp * n_nets)(*(nets if nets is not None else [_mlp(dims) for _ in range(n_nets)]))
        self.bns = self.lns = None
        if bn:
            self.bns = (_abi.GnfSntBatchNorm * max(t, 1))()
            for i in range(max(t, 1)):
                for k in ("gamma", "beta", "moving_mean", "moving_variance", "batch_mean", "batch_variance"):
                    setattr(self.bns[i], k, None if (i, k) in bn_null else P)
        if ln:
            self.lns = (_abi.GnfRowNorm * max(t, 1))()
            for i in range(max(t, 1)):
                for k in ("gamma", "beta"):
                    setattr(self.lns[i], k, None if (i, k) in ln_null else P)
        self.desc = _abi.GnfTimestepGnn(t, sharing, C.cast(self.nets, C.POINTER(_abi.GnfMlp)), _abi.GnfGnnSpec(1, combine, 2.0, 1, 0.2),
                                        C.cast(self.bns, C.POINTER(_abi.GnfSntBatchNorm)) if bn else None,
                                        C.cast(self.lns, C.POINTER(_abi.GnfRowNorm)) if ln else None, residual, training, local,
                                        eps, decay)


def test_workspace_size_is_a_host_computation_and_monotone():
    ws = _abi.lib().gnf_timestep_gnn_workspace_bytes
    e = _Enc()
    gnn = _abi.lib().gnf_gnn_workspace_bytes(100, 8, C.byref(e.nets[0]), 0)
    # fp64 moment partials [16][D][2] (256-byte aligned) | two [n, D] buffers (rounded up to 64 floats) | one module call's scratch
    assert ws(100, 8, C.byref(e.desc)) == 16 * 8 * 2 * 8 + 2 * 832 * 4 + gnn
    assert ws(100, 8, C.byref(_Enc(bn=False).desc)) == 2 * 832 * 4 + gnn
    for a, b in ((0, 1), (1, 2), (31, 32), (32, 33), (100, 101), (512, 513), (513, 70000)):
        assert ws(a, 8, C.byref(e.desc)) <= ws(b, 8, C.byref(e.desc))
    assert ws(0, 8, C.byref(e.desc)) % 4 == 0
    assert ws(-1, 8, C.byref(e.desc)) == 0 and ws(10, 0, C.byref(e.desc)) == 0 and ws(10, 8, None) == 0
    null_nets = _Enc()
    null_nets.desc.nets = None
    assert ws(10, 8, C.byref(null_nets.desc)) == 0


def _csr(n=40, e=100, b=0, off=None, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _call(enc=None, csr=None, x=P, ldx=8, out=0x100000, ldo=8, d=8, ws=P, ws_bytes=1 << 24):
    enc = _Enc() if enc is None else enc
    csr = _csr() if csr is None else csr
    return _abi.lib().gnf_timestep_gnn_f32(C.byref(csr), C.byref(enc.desc), x, ldx, out, ldo, d, ws, ws_bytes, None)


def test_validation_without_a_gpu():
    lib = _abi.lib()
    err = lambda: lib.gnf_last_error().decode()
    short = dict(ws_bytes=16)     # a call that passes every check but the last fails there: nothing ever launches on fake pointers
    assert _call(**short) == EWORKSPACE and "workspace" in err()
    # GNF_EINVAL: null arguments, bad enums, null members of a present norm entry, overlap
    assert lib.gnf_timestep_gnn_f32(None, C.byref(_Enc().desc), P, 8, 0x100000, 8, 8, P, 1 << 24, None) == EINVAL
    assert lib.gnf_timestep_gnn_f32(C.byref(_csr()), None, P, 8, 0x100000, 8, 8, P, 1 << 24, None) == EINVAL
    e = _Enc()
    e.desc.nets = None
    assert _call(e) == EINVAL
    assert _call(csr=_csr(rowptr=None)) == EINVAL and _call(csr=_csr(col=None)) == EINVAL
    e = _Enc()
    e.desc.gnn.agg = 7
    assert _call(e) == EINVAL
    for name in ("x", "out", "ws"):
        assert _call(**{name: None}) == EINVAL, name
    for key in ("gamma", "beta", "moving_mean", "moving_variance"):
        assert _call(_Enc(bn_null={(1, key)})) == EINVAL and "batch norm 1" in err(), key
    assert _call(_Enc(bn_null={(0, "batch_mean"), (2, "batch_variance")}), **short) == EWORKSPACE       # optional outputs
    moving = {(i, k) for i in range(3) for k in ("moving_mean", "moving_variance")}
    assert _call(_Enc(bn_null=moving, training=0, local=0)) == EINVAL and "moving" in err()   # evaluation reads them
    assert _call(_Enc(bn_null=moving, training=1, local=1)) == EINVAL                          # training updates them
    assert _call(_Enc(bn_null=moving, training=0, local=1), **short) == EWORKSPACE             # the one mode that needs none
    for key in ("gamma", "beta"):
        assert _call(_Enc(ln_null={(2, key)})) == EINVAL and "layer norm 2" in err(), key
    assert _call(_Enc(eps=0.0)) == EINVAL and _call(_Enc(eps=float("nan"))) == EINVAL
    assert _call(_Enc(decay=1.5)) == EINVAL and _call(_Enc(decay=-0.1)) == EINVAL
    assert _call(_Enc(decay=1.5, training=0), **short) == EWORKSPACE                           # read when training only
    assert _call(x=P, out=P) == EINVAL and "overlap" in err()
    assert _call(ws=P + 4) == EINVAL and "aligned" in err()
    assert _call(x=0x100000, out=0x100000 + 4 * (39 * 8 + 7)) == EINVAL                        # the last element of x
    assert _call(x=0x100000, out=0x100000 + 4 * (39 * 8 + 8), **short) == EWORKSPACE          # right behind it
    # graph-scope attention needs the batch's graph boundaries
    at = _abi.GnfAttn(2, 6, 5, 12, 1, 1, 0, 0, P, P, P, P, None, None, _abi.GNF_ATTN_GRAPH)
    nets = [_mlp([20, 16, 8], at) for _ in range(3)]
    assert _call(_Enc(nets=nets)) == EINVAL and "node_offsets" in err()
    assert _call(_Enc(nets=nets), csr=_csr(b=3, off=P), **short) == EWORKSPACE
    # GNF_ESHAPE: T < 1, D < 1, short strides, nets that do not map D -> D, nets of different signatures, attention geometry
    assert _call(_Enc(t=0)) == ESHAPE and "num_timesteps" in err()
    assert _call(d=0) == ESHAPE and _call(ldx=7) == ESHAPE and _call(ldo=7) == ESHAPE and "ldo" in err()
    assert _call(csr=_csr(n=-1)) == ESHAPE
    assert _call(_Enc(dims=[8, 16, 9])) == ESHAPE and "needs" in err()                         # output width
    assert _call(_Enc(dims=[16, 16, 8])) == ESHAPE                                              # input width without concat
    assert _call(_Enc(dims=[16, 16, 8], combine=1), **short) == EWORKSPACE                     # ... which concat takes
    assert _call(_Enc(dims=[8, 16, 8], combine=1)) == ESHAPE
    assert _call(_Enc(nets=[_mlp([8, 16, 8]), _mlp([8, 32, 8]), _mlp([8, 16, 8])])) == ESHAPE and "signature" in err()
    assert _call(_Enc(nets=[_mlp([8, 16, 8]), _mlp([8, 16, 16, 8]), _mlp([8, 16, 8])])) == ESHAPE
    assert _call(_Enc(sharing=1, nets=[_mlp([8, 16, 8])]), **short) == EWORKSPACE              # one net with weight sharing
    m = _mlp([8, 16, 8])
    m.num_layers = 9
    assert _call(_Enc(nets=[m, m, m])) == ESHAPE
    wide = _abi.GnfAttn(65, 6, 5, 12, 1, 1, 0, 0, P, P, P, P, None, None, _abi.GNF_ATTN_GRAPH)
    assert _call(_Enc(nets=[_mlp([20, 16, 8], wide) for _ in range(3)]), csr=_csr(b=3, off=P)) == ESHAPE
    # GNF_EUNSUPPORTED: the normalising kernel keeps two floats per column in LDS
    assert _call(_Enc(d=4097), ldx=4097, ldo=4097, d=4097) == EUNSUPPORTED
    assert _call(_Enc(d=4097, bn=False), ldx=4097, ldo=4097, d=4097, **short) == EWORKSPACE
    # n_nodes == 0: GNF_OK, no device work, whatever x / out / ws are
    assert _call(csr=_csr(n=0, e=0, rowptr=None, col=None), x=None, out=None, ws=None, ws_bytes=0) == OK
    assert _call(_Enc(t=0), csr=_csr(n=0, e=0)) == ESHAPE                                       # ... after the descriptor checks


def test_python_layer_errors_and_parameter_round_trip():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd import encoder, gnn
    assert gnf_amd.TimestepGNN is gnn.TimestepGNN and gnf_amd.evaluate is encoder.evaluate
    assert gnf_amd.write_embedding_chunks is encoder.write_embedding_chunks
    c = R.MODULE_CASES[1]                                            # avg, D = 100, BN + LN, weight sharing
    enc = encoder.make_encoder(R.family_hp(c))
    assert len(enc.gnns) == 1 and len(enc.bns) == len(enc.lns) == 3 and enc.residual is False
    assert (enc.bn_eps, enc.bn_decay_rate) == (1e-3, 0.999)
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 100), np.float32))
    for training in (False, True):
        with pytest.raises(_abi.GnfError):                           # CPU tensors: no fallback
            enc(g, training)
    with pytest.raises(_abi.GnfError):
        encoder.evaluate(enc, g)
    with pytest.raises(ValueError):
        gnn.TimestepGNN(lambda: None, 0)
    p = R.make_params(c)
    enc.set_params(p)
    back = enc.get_params()
    assert sorted(back) == ["bn", "ln", "nets"] and len(back["nets"]) == 1 and len(back["bn"]) == 3
    for (w, b), (w2, b2) in zip(p["nets"][0], back["nets"][0]):
        assert np.array_equal(w, w2) and np.array_equal(b, b2)
    for key, keys in (("bn", ("gamma", "beta", "moving_mean", "moving_variance")), ("ln", ("gamma", "beta"))):
        for a, b in zip(p[key], back[key]):
            assert all(np.array_equal(a[k], b[k]) for k in keys)
    with pytest.raises(ValueError):
        enc.set_params(dict(p, nets=p["nets"] * 2))
    with pytest.raises(ValueError):
        enc.set_params(dict(p, bn=p["bn"][:2]))


def test_an_encoder_file_round_trips(tmp_path):
    from gnf_amd import encoder
    for c in (R.MODULE_CASES[7], R.MODULE_CASES[10]):                # dm_attn BN + LN, graph-scope BN + LN with weight sharing
        hp, p = R.family_hp(c), R.make_params(c)
        enc = encoder.make_encoder(hp).set_params(p)
        path = str(tmp_path / (R.case_id(c) + ".npz"))
        encoder.save_encoder(path, hp, enc)
        enc2, hp2 = encoder.load_encoder(path)
        assert hp2 == hp and (enc2.num_timesteps, enc2.weight_sharing, enc2.residual) == (c.t, c.sharing, c.residual)
        a, b = enc.get_params(), enc2.get_params()
        for na, nb in zip(a["nets"], b["nets"]):
            assert sorted(na["attn"]) == sorted(nb["attn"]) and all(np.array_equal(na["attn"][k], nb["attn"][k]) for k in na["attn"])
            assert all(np.array_equal(w, w2) and np.array_equal(v, v2) for (w, v), (w2, v2) in zip(na["mlp"], nb["mlp"]))
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(a["bn"] + a["ln"], b["bn"] + b["ln"]) for k in x)
