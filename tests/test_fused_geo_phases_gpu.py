"""The phased instance of the compile-time-geometry half-step kernel (k_half_fused_geo<.., PHASES = true>, gnf_fused.hip):
every wave runs both nets, a layer's result stays in registers until the other net's next phase stores it, and the one
workgroup barrier of a phase sits inside it, behind those stores.  Automatic dispatch takes this instance wherever the
geometry rule holds; gnf_set_option("force_shape", 13) keeps the instance it replaces (one net per wave, a barrier per
layer) and force_shape = 12 the generic k_half_fused<1, 2>.  Which wave runs an accumulator chain and when its result is
stored is all that differs, so the three must agree bit for bit.

Every case is D = 64, T = 2 through the public flow entry point (four half-steps: the out-of-place first one, the in-place
ones, the two that also leave sum(z^2)), forward and inverse, with guard bands around source and destination.

  three-way equality (L = 256, K = 5): N = 1 (15 dead rows), 16 (one full tile), 17 (a second tile with one live row), 47 over
      three graphs (tiles that straddle graphs), a batch with an isolated node and degrees 9 - 17 (both gather rounds); mean +
      leaky_relu and sum + relu; one strided, misaligned layout.  The float64 oracle's bounds come with the shared checker.
  stale buffers: a missing or misplaced barrier shows as a layer reading what another layer (or the previous launch) left in
      an activation buffer.  N = 33 (three tiles, the last with one live row); layer j of the s-net works at 8, 4, 1/8, 2
      times its usual scale and of the t-net at 1/4, 16, 1/2, 1/16 (weights and biases scaled by powers of two, so the
      MLP's function and the exactness of the scaling are unchanged), so any two buffers differ by a factor of two at
      least.  Two runs in one process, workspace and destination refilled with NaN in between, must agree with each other
      and with force_shape = 12.
  fall-through: L = 128, K = 4 is rejected by the geometry rule and gives the generic kernel's result under 0 and 13."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import GuardBanded, graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O
from test_fused_geo_gpu import (D, DEV, K, L, LAYOUTS, NETS, T, _assert_equal_and_oracle, _hp, _problem,  # noqa: F401
                                _require_gpu_and_native_lib, _rings, force_shape)

pytestmark = pytest.mark.gpu

AUTO, PARENT, GENERIC = 0, 13, 12


def _flow_call_ws(net, graph, dst, src, direction, ws):
    """gnf_grevnet_from_f32 on a workspace the caller owns (>= the size the library asks for)."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    n, d = dst.n, dst.d
    flow = net._flow(d // 2, torch.device(DEV))
    csr = csr_desc(graph, csr_of(graph), net.graph_scope())
    ws_bytes = lib.gnf_workspace_bytes(n, d, C.byref(flow))
    assert ws.numel() >= ws_bytes
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.gnf_grevnet_from_f32(C.byref(csr), C.byref(flow), src.ptr(), src.ld, dst.ptr(), dst.ld, d, direction,
                                  _abi.ptr(sums), _abi.ptr(ws), ws_bytes, _abi.stream_ptr())
    _abi.check(rc, "gnf_grevnet_from_f32")
    torch.cuda.synchronize()
    return sums.cpu()


def _run(pr, layout, force_shape, shapes):
    """-> [(z, sums, x_back)] for each entry of `shapes` (entries may repeat), on one layout.  One workspace for all runs,
    every byte 0xFF (a NaN in every float and double) before each call; fresh NaN-banded buffers per call; guard bands checked."""
    from gnf_amd import _abi
    n, d = pr["n"], pr["d"]
    extra, c0 = layout
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = True
    graph = graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=DEV)
    out = []
    for shape in shapes:
        force_shape(shape)
        res = []
        for data, direction in ((pr["x"], _abi.GNF_FORWARD), (pr["zs"], _abi.GNF_INVERSE)):
            ws.fill_(0xFF)
            src = GuardBanded(n, d, d + extra, c0, device=DEV, fill=data)
            dst = GuardBanded(n, d, d + extra, c0, device=DEV)
            sums = _flow_call_ws(net, graph, dst, src, direction, ws)
            dst.check_guard()
            src.check_guard()
            assert torch.equal(src.window.cpu(), torch.as_tensor(data))      # the source window is read only
            res += [dst.window.cpu().clone(), sums]
        out.append((res[0], res[1], res[2]))
    return out


def _assert_same(a, b, what):
    for name, u, v in zip(("z", "[logdet, sum z^2]", "inverse x"), a, b):
        assert torch.isfinite(u).all(), f"{name}: not finite ({what})"
        assert torch.equal(u, v), f"{name}: {what}"


def _three_way(pr, layout, force_shape):
    auto, parent, generic = _run(pr, layout, force_shape, (AUTO, PARENT, GENERIC))
    _assert_same(auto, generic, "automatic dispatch vs force_shape = 12")
    _assert_same(parent, generic, "force_shape = 13 vs force_shape = 12")
    _assert_equal_and_oracle(pr, {0: auto, 12: generic})


THREE_WAY_GRAPHS = ["n1", "n16_one_graph", "n17_two_graphs", "n47_three_graphs", "isolated_and_deg9to17"]


@pytest.mark.parametrize("net", ["mean_leaky", "sum_relu"])
@pytest.mark.parametrize("gname", THREE_WAY_GRAPHS)
def test_phases_parent_and_generic_agree_bitwise(force_shape, gname, net):
    _three_way(_problem(gname, *NETS[net]), LAYOUTS["contiguous"], force_shape)


@pytest.mark.parametrize("gname,net", [("n47_three_graphs", "sum_relu"), ("isolated_and_deg9to17", "mean_leaky")])
def test_phases_on_strided_misaligned_rows(force_shape, gname, net):
    _three_way(_problem(gname, *NETS[net]), LAYOUTS["ldD+3_c3"], force_shape)


# scale of layer j's OUTPUT (hidden layers; the output layer is back at 1), per net
LAYER_SCALE = {"s": [8.0, 4.0, 0.125, 2.0, 1.0], "t": [0.25, 16.0, 0.5, 0.0625, 1.0]}


def _scaled_params(p):
    """W_j *= P_j / P_(j-1), b_j *= P_j: with a positively homogeneous activation the MLP computes what it computed, but
    layer j's activations are P_j times as large - and every factor is a power of two, so nothing is rounded."""
    out = {}
    for name in ("s", "t"):
        sc = LAYER_SCALE[name]
        out[name] = [[[(w * np.float32(sc[j] / (sc[j - 1] if j else 1.0)), b * np.float32(sc[j])) for j, (w, b) in enumerate(mlp)]
                      for mlp in half] for half in p[name]]
    return out


@pytest.mark.parametrize("net", ["mean_leaky", "sum_relu"])
def test_no_stale_activation_buffer(force_shape, net):
    agg, act = NETS[net]
    nn, ne, s, r = _rings([20, 13])
    n = int(nn.sum())
    assert n == 33 and len(LAYER_SCALE["s"]) == K
    rng = np.random.default_rng(33 + len(net))
    scale = 1.0 / np.sqrt(3.0) if agg == "sum" else 1.0
    pr = dict(hp=_hp(D, L, K, agg, act), nn=nn, ne=ne, s=s, r=r, n=n, d=D,
              x=(scale * rng.standard_normal((n, D))).astype(np.float32), zs=(scale * rng.standard_normal((n, D))).astype(np.float32),
              p=_scaled_params(O.make_grevnet_params(D + K, D // 2, L, K, T, final_scale=0.3 if agg == "mean" else 0.1)))
    first, second, generic = _run(pr, LAYOUTS["contiguous"], force_shape, (AUTO, AUTO, GENERIC))
    _assert_same(first, second, "two runs of automatic dispatch, NaN-filled workspace in between")
    _assert_same(first, generic, "automatic dispatch vs force_shape = 12")


def test_rejected_geometry_falls_through_to_the_generic_kernel(force_shape):
    pr = _problem("n47_three_graphs", "mean", "leaky_relu", latent=128, k=4)
    _three_way(pr, LAYOUTS["contiguous"], force_shape)
