"""Every entry point that takes a row stride, on node buffers that are not [N, D] contiguous: the ABI's "ONE row-major [N, D]
fp32 buffer with leading dimension ld >= D" (include/gnf.h) as a window inside a guard-banded buffer (helpers.GuardBanded).

Layouts: ld = D + 4 with the window at column 0 (the contiguous layout's alignment class), ld = D + 1 at column 1 and
ld = D + 3 at column 3 (the window's base is not 16-byte aligned, rows are not whole float4s: the kernels' scalar branches).
Every case checks
  - the guard band: every element outside the window keeps its sentinel NaN bits (no write outside the window), and the
    outputs hold no NaN (no read outside the window leaks into a result, the sums over rows included);
  - against the same call on a contiguous buffer (ld = D, column 0): bitwise where both take the same vector / scalar
    decisions (ld % 4 == 0 and column % 4 == 0), else against the float64 oracle at the suite's tolerances (1e-4 per node
    for the log-prob, the module tests' own bounds, 1e-3 of each tensor's scale for gradients).
The 2^31 crossings at the end put n * ld past 2^31 elements / bytes with a few thousand nodes and a very large ld."""
import ctypes as C
import math
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import graph_attn_ref as R
from helpers import GuardBanded, graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LN_2PI = math.log(2.0 * math.pi)
LAYOUTS = [(4, 0), (1, 1), (3, 3)]                 # (ld - D, first column of the window)
LAYOUT_IDS = ["ldD+4_c0", "ldD+1_c1", "ldD+3_c3"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()   # raises if libgnf_hip.so is missing: no silent fallback


@pytest.fixture
def options():
    """gnf_set_option for the duration of one test, every option back to automatic afterwards."""
    from gnf_amd import _abi
    touched = []

    def set_(**kw):
        for k, v in kw.items():
            _abi.set_option(k, v)
            touched.append(k)
    yield set_
    for k in touched:
        _abi.set_option(k, 0)


def _lib():
    from gnf_amd import _abi
    return _abi.lib()


def _check(rc, what):
    from gnf_amd import _abi
    _abi.check(rc, what)


def _stream():
    from gnf_amd import _abi
    return _abi.stream_ptr()


def _layout(n, d, layout, fill=None, guard=16):
    extra, c0 = layout
    return GuardBanded(n, d, d + extra, c0, guard=guard, device=DEV, fill=fill)


def _control(n, d, fill=None):
    return GuardBanded(n, d, d, 0, guard=16, device=DEV, fill=fill)


def _batch(dataset, ids):
    n_node, n_edge, sl, rl = dataset
    return O.batch_graphs(n_node, n_edge, sl, rl, ids)


def _assert_same_or_close(got, want, same, atol, rtol, what):
    """Bitwise where both runs took the same code path, else within the stated tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert not np.isnan(got).any(), f"{what}: NaN in the output (a read outside the window)"
    if same:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, atol=atol, rtol=rtol, err_msg=what)


# ---- the flow entry points: gnf_grevnet_f32 / gnf_grevnet_from_f32 ------------------------------------------------------
def _flow_call(net, graph, dst, direction, src=None):
    """gnf_grevnet_from_f32 on `dst`'s window, reading `src`'s window (None: in place, gnf_grevnet_f32).  Returns sums."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _lib()
    n, d = dst.n, dst.d
    flow = net._flow(d // 2, torch.device(DEV))
    csr = csr_desc(graph, csr_of(graph), net.graph_scope())
    ws_bytes = lib.gnf_workspace_bytes(n, d, C.byref(flow))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    if src is None:
        rc = lib.gnf_grevnet_f32(C.byref(csr), C.byref(flow), dst.ptr(), dst.ld, d, direction, _abi.ptr(sums),
                                 _abi.ptr(ws), ws_bytes, _stream())
    else:
        rc = lib.gnf_grevnet_from_f32(C.byref(csr), C.byref(flow), src.ptr(), src.ld, dst.ptr(), dst.ld, d, direction,
                                      _abi.ptr(sums), _abi.ptr(ws), ws_bytes, _stream())
    _check(rc, "gnf_grevnet_from_f32")
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def _log_prob_per_node(sums, n, d):
    return (-0.5 * float(sums[1]) - 0.5 * d * LN_2PI * n + float(sums[0])) / n


# name: (hp, dataset, graph ids, options, fused, extra)   extra: "bn", attention geometry, ...
def _hp(d, latent, k, t, agg="mean", combine="agg", eps=1.0, act="leaky_relu", ws=False, attn=None):
    hp = dict(D=d, latent=latent, K=k, T=t, agg=agg, combine=combine, epsilon=eps, activation=act, weight_sharing=ws)
    if attn is not None:
        hp.update(agg="mean", combine="agg", epsilon=0.0, activation="relu", attn=attn)
    return hp


ATTN_DEFAULT = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80, concat=True, kq_dim_division=False, residual=False)
ATTN_DATA = dict(num_heads=1, kq_dim=64, v_dim=64, out_dim=64, concat=True, kq_dim_division=True, residual=False)
ATTN_LN = dict(num_heads=3, kq_dim=7, v_dim=5, out_dim=20, concat=False, kq_dim_division=True, residual=True, layer_norm=True)
ATTN_RES = dict(num_heads=3, kq_dim=7, v_dim=5, out_dim=20, concat=False, kq_dim_division=True, residual=True)
# graph-scope attention (tests/graph_attn_ref.py): multi-head with Wo and layer norm at <1,1,8>; SelfAttention (no Wo) at <4,4,8>
GATTN_I1 = dict(scope="graph", num_heads=4, kq_dim=6, v_dim=5, out_dim=12, kq_dim_division=True, layer_norm=True)
GATTN_I4 = dict(scope="graph", num_heads=1, kq_dim=64, v_dim=64, kq_dim_division=True, layer_norm=False)


def _ghp(d, latent, k, t, attn, ws=False):
    """a graph-scope flow's hyper-parameters (graph_attn_ref.hp_of)"""
    return dict(D=d, latent=latent, K=k, T=t, agg="sum", combine="agg", epsilon=0.0, activation="relu", weight_sharing=ws,
                attn=attn)


def _is_graph(hp):
    return hp.get("attn", {}).get("scope") == "graph"


def _graph_params(seed, hp):
    a = hp["attn"]
    kw = {k: a[k] for k in ("num_heads", "kq_dim", "v_dim", "kq_dim_division", "layer_norm")}
    if "out_dim" in a:
        kw["out_dim"] = a["out_dim"]
    return R.make_graph_attn_grevnet_params(seed, hp["D"] // 2, hp["latent"], hp["K"], hp["T"],
                                            weight_sharing=hp["weight_sharing"], final_scale=0.3, **kw)

FLOW_CASES = {
    # k_half_fused at its forced shapes, both message-passing reductions and both combines
    "fused12_mean_agg": (_hp(8, 32, 3, 2), "gs", None, {"force_shape": 12}, True),
    "fused11_sum_agg": (_hp(10, 24, 2, 2, agg="sum", eps=0.5, act="relu"), "gs", None, {"force_shape": 11}, True),
    "fused21_sum_concat": (_hp(12, 24, 2, 2, agg="sum", combine="concat", eps=0.0), "gs", None, {"force_shape": 21}, True),
    "fused22_mean_concat": (_hp(16, 40, 3, 2, combine="concat", eps=0.0, ws=True), "cm", [1, 2, 3], {"force_shape": 22}, True),
    # batch norm on load (the bijector in front of every forward half-step)
    "fused_batch_norm": (_hp(8, 32, 3, 2), "gs", None, {}, True),
    "layered_batch_norm": (_hp(8, 32, 3, 2), "gs", None, {}, False),
    # k_half_big at caps 4 / 3 / 1; [10, 11] at 24 wide: four column tiles, rows split between workgroups
    "big40_split_rows": (_hp(24, 64, 3, 2, agg="sum", act="relu"), "cm", [10, 11], {"force_shape": 40}, True),
    "big30": (_hp(64, 256, 5, 2), "cm", [3, 77, 150, 9, 20], {"force_shape": 30}, True),
    "big10": (_hp(16, 48, 3, 2), "cm", [3, 77, 150], {"force_shape": 10}, True),
    # the layered path: k_aggregate, k_linear, k_linear_big / k_linear_short, k_coupling(_rows)
    "layered_mean_agg": (_hp(8, 32, 3, 2), "gs", None, {}, False),
    "layered_wide": (_hp(200, 1040, 3, 1, act="relu"), "cm", list(range(64)), {}, True),
    "layered_wide_h7": (_hp(14, 1280, 3, 1), "cm", list(range(48)), {}, True),
    # attention front-ends: the fused kernel's prologue, the rows kernels, the edge-tiled kernel, option 3
    "attn_prologue": (_hp(16, 48, 2, 2, attn=ATTN_DEFAULT), "cm", [3, 50, 77], {}, True),
    "attn_kernel1": (_hp(16, 48, 2, 2, attn=ATTN_DEFAULT), "cm", [3, 50, 77], {"attn_kernel": 1}, True),
    "attn_kernel2": (_hp(16, 48, 2, 2, attn=ATTN_DEFAULT), "cm", [3, 50, 77], {"attn_kernel": 2}, True),
    "attn_kernel3": (_hp(16, 48, 2, 2, attn=ATTN_DEFAULT), "cm", [3, 50, 77], {"attn_kernel": 3}, True),
    "attn_data_driver_head": (_hp(12, 64, 2, 1, attn=ATTN_DATA), "cm", [3, 50], {}, True),
    "attn_layer_norm": (_hp(20, 48, 2, 1, ws=True, attn=ATTN_LN), "gs", None, {}, True),
    "attn_layered_residual": (_hp(20, 48, 2, 1, attn=ATTN_RES), "gs", None, {}, False),
    # odd halves
    "odd_D2": (_hp(2, 16, 3, 2), "gs", None, {}, True),
    "odd_D6": (_hp(6, 20, 1, 2, agg="sum", combine="concat", eps=0.0), "gs", None, {}, True),
    "odd_D14": (_hp(14, 32, 2, 3), "gs", None, {}, True),
    # graph-scope attention: the front-end reads x at ldx
    "graph_attn_multihead_ln_I1": (_ghp(16, 48, 2, 2, GATTN_I1), "cm", [3, 50, 77], {}, True),
    "graph_attn_single_I4_h7": (_ghp(14, 48, 2, 1, GATTN_I4), "cm", [3, 50, 77], {}, True),
}


@lru_cache(maxsize=None)
def _flow_problem(name):
    """Batch, inputs, parameters and the float64 oracle's f(x), g(zs) of one FLOW_CASES entry (cached over layouts)."""
    from conftest import load_dataset
    hp, ds, ids, _opts, _fused = FLOW_CASES[name]
    d, k, t, ws = hp["D"], hp["K"], hp["T"], hp["weight_sharing"]
    nn, ne, s, r = _batch(load_dataset("grid_small" if ds == "gs" else "community_medium"), ids if ids else list(range(12)))
    n = int(nn.sum())
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((n, d)).astype(np.float32)
    zs = rng.standard_normal((n, d)).astype(np.float32)
    if _is_graph(hp):
        x *= 0.5
        zs *= 0.5
        p = _graph_params(d + 3, hp)
        ref = R.log_prob(nn, s, r, x, p, t, ws, activation="relu")
        xg = R.inverse(nn, s, r, zs, p, t, ws, activation="relu")
        return dict(hp=hp, nn=nn, ne=ne, s=s, r=r, n=n, x=x, zs=zs, p=p, ref=ref, xg=xg)
    if "attn" in hp:
        x *= 0.3 if hp["attn"]["residual"] else 0.5          # (a residual block adds x to s: |z| grows with it)
        zs *= 0.3 if hp["attn"]["residual"] else 0.5
        p = O.make_attn_grevnet_params(d + 3, d // 2, hp["latent"], k, t, weight_sharing=ws, final_scale=0.3, **hp["attn"])
        o = O.Fp64Dense(s, r, n, activation="relu")
    else:
        p = O.make_grevnet_params(d + k, d // 2, hp["latent"], k, t, combine=hp["combine"], weight_sharing=ws,
                                  final_scale=0.3 if hp["agg"] == "mean" else 0.1)
        o = O.Fp64Dense(s, r, n, agg=hp["agg"], combine=hp["combine"], epsilon=hp["epsilon"], activation=hp["activation"])
    if "batch_norm" in name:
        x = x * 1.5 + 0.5
        p["bn"] = O.make_bn_params(9, d // 2, t)
    ref = o.log_prob(x, p, t, ws)
    xg = o.g(zs, p, t, ws)
    return dict(hp=hp, nn=nn, ne=ne, s=s, r=r, n=n, x=x, zs=zs, p=p, ref=ref, xg=xg)


def _flow_net(name):
    pr = _flow_problem(name)
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = FLOW_CASES[name][4]
    return net, graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)


@pytest.mark.parametrize("mode", ["in_place", "from_same_ld", "from_other_ld"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_flow_forward_and_inverse(options, name, layout, mode):
    """gnf_grevnet_f32 (in place) and gnf_grevnet_from_f32 with ld_src == ld (the fused kernels' out-of-place first
    half-step) and ld_src > ld (copy, then in place), forward and inverse."""
    from gnf_amd import _abi
    pr = _flow_problem(name)
    options(**FLOW_CASES[name][3])
    n, d, x, zs = pr["n"], pr["hp"]["D"], pr["x"], pr["zs"]
    net, graph = _flow_net(name)
    extra, c0 = layout

    def src_of(data, like_ld, col):
        if mode == "in_place":
            return None
        if mode == "from_same_ld":
            return GuardBanded(n, d, like_ld, col, device=DEV, fill=data)
        return GuardBanded(n, d, like_ld + 7, 2, device=DEV, fill=data)   # ld_src > ld, another alignment

    def run(ld, col, data, direction):
        src = src_of(data, ld, col)
        dst = GuardBanded(n, d, ld, col, device=DEV, fill=data if src is None else None)
        sums = _flow_call(net, graph, dst, direction, src)
        dst.check_guard()
        if src is not None:
            src.check_guard()
            np.testing.assert_array_equal(src.numpy(), data)          # the source window is read only
        return dst.numpy(), sums

    # control: the same route on contiguous buffers (ld = D)
    z0, s0 = run(d, 0, x, _abi.GNF_FORWARD)
    xg0, _ = run(d, 0, zs, _abi.GNF_INVERSE)
    z, sums = run(d + extra, c0, x, _abi.GNF_FORWARD)
    xg, _ = run(d + extra, c0, zs, _abi.GNF_INVERSE)
    same = extra % 4 == 0 and c0 % 4 == 0 and d % 4 == 0
    assert np.isfinite(sums).all(), sums
    _assert_same_or_close(z, z0, same, 3e-4, 3e-4, "z vs contiguous")
    _assert_same_or_close(xg, xg0, same, 3e-4, 3e-4, "g(z) vs contiguous")
    if same:
        np.testing.assert_array_equal(sums, s0)
    # the float64 oracle (tolerances of test_parity_gpu.py)
    lp_tol = 1e-4
    if pr["hp"].get("attn", {}).get("layer_norm") and _is_graph(pr["hp"]):
        r32 = R.log_prob(pr["nn"], pr["s"], pr["r"], x, pr["p"], pr["hp"]["T"], pr["hp"]["weight_sharing"], activation="relu",
                         dtype=torch.float32)
        lp_tol = 1e-4 + 6.0 * abs(r32["log_prob_xs_per_node"] - pr["ref"]["log_prob_xs_per_node"])
    elif pr["hp"].get("attn", {}).get("layer_norm"):
        o32 = O.Fp32Gather(pr["s"], pr["r"], n, activation="relu")
        r32 = o32.log_prob(o32.to_t(x), o32.prep_params(pr["p"]), pr["hp"]["T"], pr["hp"]["weight_sharing"])
        lp_tol = 1e-4 + 6.0 * abs(r32["log_prob_xs_per_node"] - pr["ref"]["log_prob_xs_per_node"])
    assert abs(_log_prob_per_node(sums, n, d) - pr["ref"]["log_prob_xs_per_node"]) <= lp_tol
    np.testing.assert_allclose(z, pr["ref"]["z"], atol=3e-4, rtol=3e-4)
    np.testing.assert_allclose(xg, pr["xg"], atol=3e-4, rtol=3e-4)


# ---- gnf_coupling_half_f32 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("cond_first", [True, False], ids=["cond_first", "cond_second"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_coupling_half(grid_small, layout, cond_first, fused):
    """One half-step with the conditioning half first (x_cond = buf, x_upd = buf + H) and second (x_cond = buf + H): the
    conditioning half stays bitwise untouched, the updated half matches the oracle, the log-det is added to."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_of
    nn, ne, s, r = _batch(grid_small, [6, 7, 11])
    n, d, h = int(nn.sum()), 12, 6
    hp = _hp(d, 24, 2, 1)
    p = O.make_grevnet_params(8, h, 24, 2, 1, final_scale=0.5)
    x = np.random.default_rng(8).standard_normal((n, d)).astype(np.float32)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    g = graph_from_arrays(nn, ne, s, r, x, DEV)
    flow = net._flow(h, torch.device(DEV))
    csr = csr_of(g)
    lib = _lib()
    ws_bytes = lib.gnf_workspace_bytes(n, d, C.byref(flow))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    cc, uc = (0, h) if cond_first else (h, 0)

    def run(buf, direction, acc):
        _check(lib.gnf_coupling_half_f32(C.byref(csr.desc), C.byref(flow.s_nets[0]), C.byref(flow.t_nets[0]),
                                         C.byref(flow.gnn), buf.ptr(cc), buf.ptr(uc), buf.ld, h, direction,
                                         _abi.ptr(acc), _abi.ptr(ws), ws_bytes, _stream()), "gnf_coupling_half_f32")
        torch.cuda.synchronize()
        buf.check_guard()
        return buf.numpy()

    ctl = _control(n, d, x)
    acc0 = torch.full((1,), 10.0, dtype=torch.float64, device=DEV)
    y0 = run(ctl, _abi.GNF_FORWARD, acc0)
    buf = _layout(n, d, layout, x)
    acc = torch.full((1,), 10.0, dtype=torch.float64, device=DEV)
    y = run(buf, _abi.GNF_FORWARD, acc)
    np.testing.assert_array_equal(y[:, cc:cc + h], x[:, cc:cc + h])          # conditioning half untouched
    o = O.Fp64Dense(s, r, n, agg="mean", epsilon=1.0, activation="leaky_relu")
    xc = x[:, cc:cc + h].astype(np.float64)
    sv, tv = o.gnn(xc, p["s"][0][0]), o.gnn(xc, p["t"][0][0])
    np.testing.assert_allclose(y[:, uc:uc + h], x[:, uc:uc + h] * np.exp(sv) + tv, atol=1e-5, rtol=1e-5)
    assert abs(float(acc[0]) - (10.0 + sv.sum())) < 1e-4
    same = buf.aligned()
    _assert_same_or_close(y, y0, same, 1e-5, 1e-5, "coupling vs contiguous")
    if same:
        assert float(acc[0]) == float(acc0[0])
    back = run(buf, _abi.GNF_INVERSE, None)
    np.testing.assert_array_equal(back[:, cc:cc + h], x[:, cc:cc + h])
    np.testing.assert_allclose(back, x, atol=1e-5, rtol=1e-5)


# ---- gnf_aggregate_f32 / gnf_gnn_apply_f32: ldx != ldo ----------------------------------------------------------------
OUT_LAYOUTS = {(4, 0): (8, 4), (1, 1): (5, 2), (3, 3): (2, 1)}               # the output's (ld - width, column)


@pytest.mark.parametrize("agg", ["sum", "mean"])
@pytest.mark.parametrize("h", [1, 3, 32, 300])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_aggregate(layout, h, agg):
    from gnf_amd.graphs import csr_of
    from gnf_amd import _abi
    from test_parity_gpu import _hub_graphs
    nn, ne, s, r = _hub_graphs(h)
    n = int(nn.sum())
    x = np.random.default_rng(h).standard_normal((n, h)).astype(np.float32)
    csr = csr_of(graph_from_arrays(nn, ne, s, r, x, DEV))
    code = _abi.GNF_AGG_MEAN if agg == "mean" else _abi.GNF_AGG_SUM

    def run(xb, ob):
        _check(_lib().gnf_aggregate_f32(C.byref(csr.desc), xb.ptr(), xb.ld, h, code, ob.ptr(), ob.ld, _stream()),
               "gnf_aggregate_f32")
        torch.cuda.synchronize()
        xb.check_guard()
        ob.check_guard()
        np.testing.assert_array_equal(xb.numpy(), x)
        return ob.numpy()

    want0 = run(_control(n, h, x), _control(n, h))
    xb, ob = _layout(n, h, layout, x), _layout(n, h, OUT_LAYOUTS[layout])
    assert xb.ld != ob.ld
    got = run(xb, ob)
    deg = np.bincount(r, minlength=n).astype(np.float64)
    want = np.zeros((n, h))
    np.add.at(want, r, x.astype(np.float64)[s])
    if agg == "mean":
        want = want / np.maximum(deg, 1.0)[:, None]
    np.testing.assert_allclose(got, want, atol=3e-5 * (1.0 if agg == "mean" else 20.0), rtol=1e-5)
    _assert_same_or_close(got, want0, xb.aligned() and ob.aligned(), 3e-5 * (1.0 if agg == "mean" else 20.0), 1e-5,
                          "aggregate vs contiguous")


def _gnn_apply(mod, graph, xb, ob):
    """gnf_gnn_apply_f32 with the caller's strides: the module call of gnn.py (_NodeBlock._build) on explicit buffers."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _lib()
    h = xb.d
    mlp = mod._node_block._mlp if hasattr(mod, "_node_block") else mod._mlp
    blk = mod._node_block if hasattr(mod, "_node_block") else mod
    mlp = blk._mlp.ensure_built(blk.in_dim(h), torch.device(DEV))
    desc = _abi.GnfMlp()
    mlp.fill_desc(desc, 0)
    attn = blk.attn_desc(h, torch.device(DEV))
    if attn is not None:
        desc.attn = C.pointer(attn)
    spec = blk.spec()
    csr = csr_desc(graph, csr_of(graph), blk.graph_scope)
    n = xb.n
    ws_bytes = lib.gnf_gnn_workspace_bytes(n, h, C.byref(desc), spec.combine)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=DEV)
    _check(lib.gnf_gnn_apply_f32(C.byref(csr), C.byref(desc), C.byref(spec), xb.ptr(), xb.ld, h, ob.ptr(), ob.ld,
                                 _abi.ptr(ws), ws_bytes, _stream()), "gnf_gnn_apply_f32")
    torch.cuda.synchronize()
    xb.check_guard()
    ob.check_guard()
    return ob.numpy()


GNN_APPLY_CASES = ["agg_narrow", "concat_wide", "attention", "attention_layer_norm", "graph_attn_multihead_ln_I1",
                   "graph_attn_single_I4_h13"]


@pytest.mark.parametrize("case", GNN_APPLY_CASES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_gnn_apply(layout, case):
    from gnf_amd import gnn
    from test_parity_gpu import _hub_graphs
    nn, ne, s, r = _hub_graphs(11)
    n = int(nn.sum())
    h, od = (13 if case.endswith("_h13") else 12), 7
    x = np.random.default_rng(5).standard_normal((n, h)).astype(np.float32)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    if case in ("agg_narrow", "concat_wide"):
        latent = 1100 if case == "concat_wide" else 24
        in0 = 2 * h if case == "concat_wide" else h
        layers = O.make_mlp_params(np.random.default_rng(6), in0, latent, od, 2)
        mk = partial(gnn.make_mlp_model, latent, od, 2, gnn.leaky_relu)
        mod = gnn.sum_concat_then_mlp_gnn(mk) if case == "concat_wide" else gnn.avg_then_mlp_gnn(mk, 0.5)
        mod._node_block._mlp.set_params(layers)
        o = O.Fp64Dense(s, r, n, agg="sum" if case == "concat_wide" else "mean",
                        combine="concat" if case == "concat_wide" else "agg", epsilon=0.5)
        want = o.gnn(x.astype(np.float64), layers)
        tol = 2e-4
    elif case.startswith("graph_attn"):
        single = case.endswith("_h13")
        g = {k: v for k, v in (GATTN_I4 if single else GATTN_I1).items() if k != "scope"}
        net = R.make_graph_attn_net_params(np.random.default_rng(1), h, 16, 2, **g)
        net["mlp"] = O.make_mlp_params(np.random.default_rng(2), h + (g["v_dim"] if single else g["out_dim"]), 16, od, 2)
        if not single:                                                 # (layer norm over the MLP's od outputs)
            net["attn"].update(ln_gamma=np.linspace(0.5, 1.5, od).astype(np.float32),
                               ln_beta=np.linspace(-0.3, 0.3, od).astype(np.float32))
        mk = partial(gnn.make_mlp_model, 16, od, 2, gnn.relu)
        mod = gnn.self_attn_gnn(g["kq_dim"], g["v_dim"], mk, True) if single else \
            gnn.multihead_self_attn_gnn(g["kq_dim"], g["v_dim"], g["out_dim"], mk, num_heads=g["num_heads"], layer_norm=True)
        mod.set_attn_params(net["attn"])
        mod._mlp.set_params(net["mlp"])
        o = R.GraphAttnGather(s, r, nn, activation="relu")
        want = o.attn_gnn(o.to_t(x), o.prep_params({"n": [net]})["n"][0]).numpy()
        tol = 1e-4
    else:
        ln = case == "attention_layer_norm"
        net = O.make_attn_net_params(np.random.default_rng(1), h, 16, 2, num_heads=4, kq_dim=3, v_dim=2, out_dim=5)
        net["mlp"] = O.make_mlp_params(np.random.default_rng(2), h + 5, 16, od, 2)
        mod = gnn.dm_self_attn_gnn(kq_dim=3, v_dim=2, make_mlp_fn=partial(gnn.make_mlp_model, 16, od, 2, gnn.relu),
                                   num_heads=4, concat_heads_output_dim=5, layer_norm=ln)
        mod(graph)                                                     # first connection creates the variables
        if ln:
            net["attn"].update(layer_norm=True, ln_gamma=np.linspace(0.5, 1.5, od).astype(np.float32),
                               ln_beta=np.linspace(-0.3, 0.3, od).astype(np.float32))
        mod.set_attn_params(net["attn"])
        mod._mlp.set_params(net["mlp"])
        want = O.Fp64Dense(s, r, n, activation="relu").gnn(x.astype(np.float64), net)
        tol = 1e-4
    ref0 = mod(graph).nodes.cpu().numpy()                              # the product's own call (contiguous)
    ctl = _gnn_apply(mod, graph, _control(n, h, x), _control(n, od))
    np.testing.assert_array_equal(ctl, ref0)
    xb, ob = _layout(n, h, layout, x), _layout(n, od, OUT_LAYOUTS[layout])
    got = _gnn_apply(mod, graph, xb, ob)
    np.testing.assert_array_equal(xb.numpy(), x)
    np.testing.assert_allclose(got, want, atol=tol, rtol=tol)
    _assert_same_or_close(got, ctl, xb.aligned() and ob.aligned() and od % 4 == 0, tol, tol, "gnn_apply vs contiguous")


# ---- gnf_pred_adj_f32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 1100], ids=["lds_rows", "global_rows"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_pred_adj(layout, d):
    from gnf_amd import _abi
    from gnf_amd.flow import pred_adj, scaled_hacky_sigmoid_l2
    rng = np.random.default_rng(d)
    n_node = np.array([17, 1, 40, 33], np.int32)
    n = int(n_node.sum())
    z = (rng.standard_normal((n, d)) * (0.7 if d < 1000 else 0.12)).astype(np.float32)
    g = graph_from_arrays(n_node, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z, DEV)
    ctl = torch.cat([b.flatten() for b in pred_adj(g, distance_fn=scaled_hacky_sigmoid_l2)]).cpu().numpy()
    lib = _lib()
    zb = _layout(n, d, layout, z)
    total = int((n_node.astype(np.int64) ** 2).sum())
    out = torch.full((total,), float("nan"), device=DEV)
    off = torch.empty(5, dtype=torch.int64, device=DEV)
    ws_bytes = lib.gnf_pred_adj_workspace_bytes(4)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    nn = torch.as_tensor(n_node).to(DEV)
    _check(lib.gnf_pred_adj_f32(zb.ptr(), zb.ld, d, _abi.ptr(nn), 4, 64, _abi.ptr(out), _abi.ptr(off), _abi.ptr(ws),
                                ws_bytes, _stream()), "gnf_pred_adj_f32")
    torch.cuda.synchronize()
    zb.check_guard()
    got = out.cpu().numpy()
    want = np.concatenate([b.ravel() for b in O.pred_adj_blocks(z, n_node)])
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-4)
    _assert_same_or_close(got, ctl, zb.aligned(), 2e-5, 1e-4, "pred_adj vs contiguous")


# ---- gnf_gauss_sumsq_f32 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_gauss_sumsq(layout):
    from gnf_amd import _abi
    z = np.random.default_rng(6).standard_normal((1234, 10)).astype(np.float32)
    zb = _layout(1234, 10, layout, z)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(8 * 1024, dtype=torch.uint8, device=DEV)
    _check(_lib().gnf_gauss_sumsq_f32(zb.ptr(), 1234, 10, zb.ld, _abi.ptr(out), _abi.ptr(ws), 8 * 1024, _stream()),
           "gnf_gauss_sumsq_f32")
    torch.cuda.synchronize()
    zb.check_guard()
    assert abs(float(out[0]) - float((z.astype(np.float64) ** 2).sum())) < 1e-8 * float(out[0])


# ---- gnf_grevnet_backward_f32 -------------------------------------------------------------------------------------------
def _strided_loss_and_grads(tr, graph, src, z):
    """GRevNetTrainer.loss_and_grads / _loss_and_grads (train.py), with the forward pass reading `src`'s window and leaving
    z in `z`'s window, and the backward walk run in place on that window.  The gradient lands in tr.grad; returns sums."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _lib()
    net = tr.net
    n, d = z.n, z.d
    dev = torch.device(DEV)
    tr._ensure_arena(d // 2, dev)
    fwd_flow = net._flow(d // 2, dev)
    stash_bytes = lib.gnf_attn_stash_bytes(n, d, C.byref(fwd_flow)) if tr.stash_attention else 0
    mlp_bytes = lib.gnf_mlp_stash_bytes(n, d, C.byref(fwd_flow)) if tr.stash_mlp_rows else 0
    if stash_bytes:
        if tr._stash is None or tr._stash.numel() < stash_bytes:
            tr._stash = torch.empty(stash_bytes, dtype=torch.uint8, device=dev)
        fwd_flow.attn_stash, fwd_flow.attn_stash_bytes = tr._stash.data_ptr(), stash_bytes
    if mlp_bytes and not tr._ensure_mlp_stash(mlp_bytes, dev):
        mlp_bytes = 0
    if mlp_bytes:
        fwd_flow.mlp_stash, fwd_flow.mlp_stash_bytes = tr._mlp_stash.data_ptr(), mlp_bytes
    try:
        sums = _flow_call(net, graph, z, _abi.GNF_FORWARD, src)
        flow = net._flow(d // 2, dev)
        csr, csr_t = csr_desc(graph, csr_of(graph), net.graph_scope()), csr_of(graph, by_sender=True)
        ws_bytes = lib.gnf_backward_workspace_bytes(n, d, C.byref(flow))
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        aux = torch.cuda.Stream(device=dev) if tr.overlap_weight_grads else None
        _check(lib.gnf_grevnet_backward_f32(C.byref(csr), C.byref(csr_t.desc), C.byref(flow), C.byref(tr._grad_flow),
                                            z.ptr(), z.ld, d, _abi.ptr(ws), ws_bytes, _stream(),
                                            C.c_void_p(aux.cuda_stream if aux is not None else 0)),
               "gnf_grevnet_backward_f32")
        torch.cuda.synchronize()
    finally:
        fwd_flow.attn_stash, fwd_flow.attn_stash_bytes = None, 0
        fwd_flow.mlp_stash, fwd_flow.mlp_stash_bytes = None, 0
    return sums


def _flatten(tree, path=""):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flatten(tree[k], f"{path}.{k}")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from _flatten(v, f"{path}[{i}]")
    else:
        yield path, np.asarray(tree)


def _check_grads_vs_oracle(got, ref, scale=1e-3, norm=False):
    pairs = list(zip(_flatten(got), _flatten(ref)))
    gmax = max(float(np.abs(b).max()) for _, (_, b) in pairs)
    for (name, a), (name_r, b) in pairs:
        assert name == name_r and a.shape == b.shape, (name, name_r)
        assert not np.isnan(a).any(), f"{name}: NaN"
        if norm:   # (wide nets: single elements next to a relu kink of the reconstruction may land on the other side)
            bound = 2e-3 * max(float(np.linalg.norm(b)), 1e-3 * gmax * np.sqrt(b.size))
            assert float(np.linalg.norm(a - b)) <= bound, name
        else:
            tol = scale * float(np.abs(b).max()) + 1e-5 + 1e-6 * gmax
            err = float(np.abs(a - b).max())
            assert err <= tol, f"{name}: max err {err:.3e} > {tol:.3e}"


BWD_CASES = {
    # name: (hp, dataset, ids, options, fused, stash, batch norm)
    "fused_stash": (_hp(8, 32, 3, 2), "gs", None, {}, True, True, False),
    "fused_recompute": (_hp(12, 48, 3, 2, combine="concat", eps=0.0, ws=True), "gs", None, {}, True, False, False),
    "bwd_generic": (_hp(8, 32, 3, 2), "gs", None, {"bwd_generic": 1}, True, False, False),
    "dw_grouped": (_hp(10, 24, 2, 2, agg="sum", eps=0.5), "gs", None, {"dw_grouped": 1}, True, False, False),
    "gemm_path": (_hp(8, 32, 3, 2), "gs", None, {}, False, False, False),
    "batch_norm": (_hp(8, 32, 3, 2), "gs", None, {}, True, False, True),
    "attn_stash": (_hp(12, 32, 3, 1, attn=ATTN_RES), "cm", [3, 50, 77], {}, True, True, False),
    "attn_recompute_rows": (_hp(16, 48, 2, 2, attn=ATTN_DEFAULT), "cm", [3, 50, 77], {"attn_kernel": 1}, True, False, False),
    "wide_dw": (_hp(14, 1280, 3, 1), "cm", list(range(24)), {"dw_wide_units": 64}, True, True, False),
    # graph-scope attention: the front-end reads x at ldx, the dL/dx kernel reads x_cond at xc_ld and adds into g at ldg
    "graph_attn_multihead_ln_I1": (_ghp(16, 48, 2, 2, GATTN_I1), "cm", [3, 50, 77], {}, True, True, False),
    "graph_attn_single_I4_h7": (_ghp(14, 48, 2, 1, GATTN_I4), "cm", [3, 50, 77], {}, True, False, False),
}


@lru_cache(maxsize=None)
def _bwd_problem(name):
    from conftest import load_dataset
    hp, ds, ids, _o, _f, _st, bn = BWD_CASES[name]
    d, k, t, ws = hp["D"], hp["K"], hp["T"], hp["weight_sharing"]
    nn, ne, s, r = _batch(load_dataset("grid_small" if ds == "gs" else "community_medium"), ids if ids else list(range(12)))
    n = int(nn.sum())
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if _is_graph(hp):
        x *= 0.3
        p = _graph_params(d + 1, hp)
        ref = R.loss_and_grads(nn, s, r, x, p, t, ws, activation="relu")
    elif "attn" in hp:
        x *= 0.3
        p = O.make_attn_grevnet_params(d + 1, d // 2, hp["latent"], k, t, weight_sharing=ws, final_scale=0.3, **hp["attn"])
        ref = O.loss_and_grads(s, r, n, x, p, t, ws, activation="relu")
    else:
        if bn:
            x = x * 1.5 + 0.5
        p = O.make_grevnet_params(d + k, d // 2, hp["latent"], k, t, combine=hp["combine"], weight_sharing=ws,
                                  final_scale=0.3 if hp["agg"] == "mean" else 0.1)
        if bn:
            p["bn"] = O.make_bn_params(9, d // 2, t)
        ref = O.loss_and_grads(s, r, n, x, p, t, ws, agg=hp["agg"], combine=hp["combine"], epsilon=hp["epsilon"],
                               activation=hp["activation"])
    return dict(hp=hp, nn=nn, ne=ne, s=s, r=r, n=n, x=x, p=p, ref=ref)


def _trainer(name):
    from gnf_amd.train import GRevNetTrainer
    pr = _bwd_problem(name)
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = BWD_CASES[name][4]
    tr = GRevNetTrainer(net)
    tr.stash_attention = tr.stash_mlp_rows = BWD_CASES[name][5]
    return tr, graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_backward(options, name, layout):
    """z in a guard-banded buffer through the forward pass and gnf_grevnet_backward_f32: the gradients against the
    contiguous run and the fp64 autograd oracle, the reconstruction inside the window."""
    pr = _bwd_problem(name)
    options(**BWD_CASES[name][3])
    n, d, x = pr["n"], pr["hp"]["D"], pr["x"]
    tr, graph = _trainer(name)
    tr.loss_and_grads(graph)                                          # the product's own step (contiguous)
    torch.cuda.synchronize()
    g_product = tr.grad.clone()
    src0, z0 = _control(n, d, x), _control(n, d)
    s0 = _strided_loss_and_grads(tr, graph, src0, z0)
    g0 = tr.grad.clone()
    assert torch.equal(g0, g_product)                                 # the mirror of _loss_and_grads is the product
    src, z = _layout(n, d, layout, x), _layout(n, d, layout)
    sums = _strided_loss_and_grads(tr, graph, src, z)
    g = tr.grad.clone()
    for b in (src, z):
        b.check_guard()
    np.testing.assert_array_equal(src.numpy(), x)
    assert np.isfinite(sums).all() and not torch.isnan(g).any()
    same = src.aligned()
    if same:
        assert torch.equal(g, g0)
        np.testing.assert_array_equal(sums, s0)
        np.testing.assert_array_equal(z.numpy(), z0.numpy())
    else:
        gs, gc = g.cpu().numpy(), g0.cpu().numpy()
        assert np.abs(gs - gc).max() <= 1e-3 * max(np.abs(gc).max(), 1e-12)
    total_loss = 0.5 * float(sums[1]) + 0.5 * d * LN_2PI * n - float(sums[0])
    assert abs(total_loss - pr["ref"]["total_loss"]) <= 1e-4 * n
    np.testing.assert_allclose(z.numpy(), x, atol=3e-4, rtol=3e-4)     # the reconstruction, in the window
    _check_grads_vs_oracle(tr.named_gradients(), pr["ref"]["grads"], norm=name == "wide_dw")


# ---- the Python surface on column views of a wider tensor ---------------------------------------------------------------
def test_python_surface_on_column_views(grid_small):
    """GRevNet.f / .g / log_prob, sample -> pred_adj and one trainer step on wide[:, 3:3 + D] views against the same data
    passed contiguously.  A view goes through gnf_grevnet_from_f32 with ld_src = 3 + D + 5 != ld (copy, then in place), a
    contiguous tensor through the fused kernel's out-of-place first half-step: the same arithmetic per element."""
    from gnf_amd.flow import log_prob_terms, pred_adj, scaled_hacky_sigmoid_l2
    from gnf_amd.train import GRevNetTrainer
    nn, ne, s, r = _batch(grid_small, list(range(12)))
    n, d = int(nn.sum()), 8
    hp = _hp(d, 32, 3, 2)
    p = O.make_grevnet_params(3, d // 2, 32, 3, 2, final_scale=0.3)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, d)).astype(np.float32)
    wide = torch.full((n, d + 8), float("nan"), device=DEV)
    wide[:, 3:3 + d] = torch.as_tensor(x).to(DEV)
    view = wide[:, 3:3 + d]
    assert view.stride() == (d + 8, 1)
    gv = graph_from_arrays(nn, ne, s, r, x, DEV).replace(nodes=view)
    gc = graph_from_arrays(nn, ne, s, r, x, DEV)
    net = make_product_grevnet(hp, p)
    zv, ldv = net.f(gv)
    zc, ldc = net.f(gc)
    assert torch.equal(zv.nodes, zc.nodes) and float(ldv) == float(ldc)
    wz = torch.full((n, d + 8), float("nan"), device=DEV)
    wz[:, 3:3 + d] = zc.nodes
    assert torch.equal(net.g(gc.replace(nodes=wz[:, 3:3 + d])).nodes, net.g(zc).nodes)
    assert torch.equal(net.log_prob(gv), net.log_prob(gc))
    lt = log_prob_terms(net, gv)
    ref = O.Fp64Dense(s, r, n, agg="mean", epsilon=1.0, activation="leaky_relu").log_prob(x, p, 2)
    assert abs(float(lt["log_prob_xs_per_node"]) - ref["log_prob_xs_per_node"]) <= 1e-4
    # sampling direction, then the decoder on a view of its output
    xs = net.g(gc.replace(nodes=wz[:, 3:3 + d])).nodes
    wx = torch.full((n, d + 8), float("nan"), device=DEV)
    wx[:, 3:3 + d] = xs
    bv = pred_adj(gc.replace(nodes=wx[:, 3:3 + d]), distance_fn=scaled_hacky_sigmoid_l2)
    bc = pred_adj(gc.replace(nodes=xs), distance_fn=scaled_hacky_sigmoid_l2)
    assert all(torch.equal(a, b) for a, b in zip(bv, bc))
    # one trainer step
    steps = []
    for graph in (gv, gc):
        tr = GRevNetTrainer(make_product_grevnet(hp, p))
        out = tr.step(graph)
        torch.cuda.synchronize()
        steps.append((tr.theta.clone(), float(out["total_loss"])))
    assert torch.equal(steps[0][0], steps[1][0]) and steps[0][1] == steps[1][1]
    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + d:]).all()


# ---- the 2^31 crossings -------------------------------------------------------------------------------------------------
def _need_bytes_or_skip(nbytes):
    free, _total = torch.cuda.mem_get_info()
    if free < 2 * nbytes:
        pytest.skip(f"needs twice {nbytes / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")


def test_n_times_ld_past_2_31_elements_big_kernel_steps_aside(community_medium, options):
    """n * ld >= 2^31 elements (k_half_big's coupling loop indexes rows with 32-bit offsets: choose_big in gnf_fused.hip
    turns it off there) with force_shape = 40 asking for it: the regular fused kernel runs, forward and inverse match the
    oracle, the guard band is intact."""
    from gnf_amd import _abi
    nn, ne, s, r = _batch(community_medium, list(range(100)))
    n, d = int(nn.sum()), 16
    ld = (2 ** 31) // n + 3                                              # odd: scalar loads; n * ld > 2^31
    assert n * ld >= 2 ** 31 and 2048 <= n <= 8192
    _need_bytes_or_skip((n + 32) * ld * 4)
    hp = _hp(d, 32, 2, 2)
    p = O.make_grevnet_params(31, d // 2, 32, 2, 2, final_scale=0.3)
    x = np.random.default_rng(31).standard_normal((n, d)).astype(np.float32)
    o = O.Fp64Dense(s, r, n, agg="mean", epsilon=1.0, activation="leaky_relu")
    ref = o.log_prob(x, p, 2)
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    options(force_shape=40)
    buf = GuardBanded(n, d, ld, 1, device=DEV, fill=x)
    sums = _flow_call(net, graph, buf, _abi.GNF_FORWARD)
    z = buf.numpy()
    buf.check_guard()
    assert abs(_log_prob_per_node(sums, n, d) - ref["log_prob_xs_per_node"]) <= 1e-4
    np.testing.assert_allclose(z, ref["z"], atol=3e-4, rtol=3e-4)
    _flow_call(net, graph, buf, _abi.GNF_INVERSE)
    buf.check_guard()
    np.testing.assert_allclose(buf.numpy(), x, atol=3e-4, rtol=3e-4)
    buf.release()
    del buf
    torch.cuda.empty_cache()


def test_n_times_ld_past_2_31_bytes_wide_forward_and_backward(community_medium):
    """n * ld * 4 >= 2^31 bytes on a net too wide for the fused kernels (the layered forward and the GEMM backward walk,
    whose buffer-descriptor guards in gnf_linear_big.hip / gnf_train.hip are sized by the workspace strides, not by ld):
    every kernel that indexes the caller's buffer does so in 64 bits.  Loss and gradients vs the oracle, reconstruction and
    guard band."""
    from gnf_amd.train import GRevNetTrainer
    nn, ne, s, r = _batch(community_medium, list(range(40)))
    n, d = int(nn.sum()), 14
    ld = (2 ** 31) // (4 * n) + 1
    assert n * ld * 4 >= 2 ** 31 and n * ld < 2 ** 31 and 1024 <= n <= 8192
    _need_bytes_or_skip(2 * (n + 32) * ld * 4)
    hp = _hp(d, 1280, 3, 1)
    p = O.make_grevnet_params(51, d // 2, 1280, 3, 1, final_scale=0.3)
    x = (np.random.default_rng(9).standard_normal((n, d)) * 0.7).astype(np.float32)
    ref = O.loss_and_grads(s, r, n, x, p, 1, activation="leaky_relu")
    tr = GRevNetTrainer(make_product_grevnet(hp, p))
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    src = GuardBanded(n, d, ld, 3, device=DEV, fill=x)
    z = GuardBanded(n, d, ld, 3, device=DEV)
    sums = _strided_loss_and_grads(tr, graph, src, z)
    for b in (src, z):
        b.check_guard()
    total_loss = 0.5 * float(sums[1]) + 0.5 * d * LN_2PI * n - float(sums[0])
    assert abs(total_loss - ref["total_loss"]) <= 1e-4 * n
    np.testing.assert_allclose(z.numpy(), x, atol=3e-4, rtol=3e-4)
    _check_grads_vs_oracle(tr.named_gradients(), ref["grads"], norm=True)
    src.release()
    z.release()
    del src, z
    torch.cuda.empty_cache()
