"""The compile-time-geometry instance of the fused half-step kernel (k_half_fused_geo, gnf_fused.hip) against the generic
instance it replaces.

launch_half_fused takes the new instance for the message-passing GNN at in0 = H = 32, L = 256, K = 5, combine = agg when no
shape is forced; gnf_set_option("force_shape", 12) keeps the generic k_half_fused<1, 2> in the same binary.  Every case runs
the public flow entry points twice in one process - force_shape = 0, then 12 - at T = 2 (four half-steps: the out-of-place
first one, the in-place ones, the two that also leave sum(z^2)) and asserts torch.equal on z, on [logdet, sum z^2] and, in
the inverse direction, on x; then the suite's 1e-4 per-node log-prob bound against the float64 oracle.

Shapes: the smallest at which this kernel can go wrong - one row; one full tile; a last tile with one live row; graph
boundaries inside tiles; a node without incoming edges (max(deg, 1)); nodes of degree 9 - 17 (two gather rounds); one
complete graph of 140 nodes with self loops (a tile's column segment of 2 240 > the LDS slice of 2 048: the gather reads
`col` from global memory); a row stride above D with a base off 16-byte alignment."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

from helpers import GuardBanded, graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LN_2PI = math.log(2.0 * math.pi)
D, L, K, T = 64, 256, 5, 2


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()   # raises if libgnf_hip.so is missing: no silent fallback


@pytest.fixture
def force_shape():
    from gnf_amd import _abi
    yield lambda v: _abi.set_option("force_shape", v)
    _abi.set_option("force_shape", 0)


# ---- graphs: (n_node, n_edge, senders, receivers), nodes numbered over the batch ----------------------------------------
def _ring(n, first, self_loops=True):
    """A ring of n nodes from node `first` on, both directions, plus self loops (n = 1: the self loop alone)."""
    s, r = [], []
    for i in range(n):
        if self_loops:
            s.append(first + i), r.append(first + i)
        if n > 1:
            s.append(first + i), r.append(first + (i + 1) % n)
            if n > 2:
                s.append(first + (i + 1) % n), r.append(first + i)
    return s, r


def _batch_of(parts):
    """parts: per graph (n, senders, receivers) with batch-wide node numbers"""
    nn = np.array([p[0] for p in parts], np.int32)
    ne = np.array([len(p[1]) for p in parts], np.int32)
    s = np.concatenate([np.asarray(p[1], np.int32) for p in parts])
    r = np.concatenate([np.asarray(p[2], np.int32) for p in parts])
    return nn, ne, s, r


def _rings(sizes):
    parts, first = [], 0
    for n in sizes:
        s, r = _ring(n, first)
        parts.append((n, s, r))
        first += n
    return _batch_of(parts)


def _degrees():
    """One graph of 40 nodes: node 0 has no incoming edge (and no self loop), node v in 1 .. 9 receives from 8 + v distinct
    senders (degrees 9 .. 17: a full gather round of 8 and a tail of 1 .. 7, then two full rounds, then 2 x 8 + 1), the rest
    form a ring; edges are listed sender-major, so a receiver's edges are not contiguous in the input."""
    n = 40
    pairs = []
    for v in range(1, 10):
        for q in range(8 + v):
            pairs.append(((v + 3 + 2 * q) % n, v))
    rs, rr = _ring(30, 10, self_loops=False)
    pairs += list(zip(rs, rr))
    pairs = [p for p in pairs if p[1] != 0]
    pairs.sort()
    return _batch_of([(n, [p[0] for p in pairs], [p[1] for p in pairs])])


def _complete(n):
    idx = np.arange(n, dtype=np.int32)
    return _batch_of([(n, np.repeat(idx, n), np.tile(idx, n))])


GRAPHS = {
    "n1": lambda: _rings([1]),
    "n16_one_graph": lambda: _rings([16]),
    "n17_two_graphs": lambda: _rings([9, 8]),
    "n47_three_graphs": lambda: _rings([13, 21, 13]),
    "isolated_and_deg9to17": _degrees,
    "complete140": lambda: _complete(140),
}
NETS = {   # name: (agg, activation)
    "mean_leaky": ("mean", "leaky_relu"),
    "sum_relu": ("sum", "relu"),
    "sum_leaky": ("sum", "leaky_relu"),
    "mean_relu": ("mean", "relu"),
}
# (ld - D, first column of the window): contiguous; a row stride above D at the contiguous alignment; a base 12 bytes off
# 16-byte alignment with rows that are not whole float4s
LAYOUTS = {"contiguous": (0, 0), "ldD+4_c0": (4, 0), "ldD+3_c3": (3, 3)}


def _hp(d, latent, k, agg, act, combine="agg"):
    return dict(D=d, latent=latent, K=k, T=T, agg=agg, combine=combine, epsilon=1.0 if combine == "agg" else 0.0,
                activation=act, weight_sharing=False)


@lru_cache(maxsize=None)
def _problem(gname, agg, act, d=D, latent=L, k=K, combine="agg"):
    """Batch, inputs, parameters and the float64 oracle's log-prob of x and g(zs): computed once, shared by the layouts."""
    nn, ne, s, r = GRAPHS[gname]()
    n = int(nn.sum())
    hp = _hp(d, latent, k, agg, act, combine)
    rng = np.random.default_rng(sum(map(ord, gname + agg + act)) + d + latent + k)
    # (a sum over up to 140 neighbours: inputs scaled so that the layer-0 rows, and with them s, stay O(1))
    scale = 1.0 / math.sqrt(float(max(1, int(np.bincount(r, minlength=n).max())))) if agg == "sum" else 1.0
    x = (scale * rng.standard_normal((n, d))).astype(np.float32)
    zs = (scale * rng.standard_normal((n, d))).astype(np.float32)
    p = O.make_grevnet_params(d + k, d // 2, latent, k, T, combine=combine, final_scale=0.3 if agg == "mean" else 0.1)
    o = O.Fp64Dense(s, r, n, agg=agg, combine=combine, epsilon=hp["epsilon"], activation=act)
    return dict(hp=hp, nn=nn, ne=ne, s=s, r=r, n=n, d=d, x=x, zs=zs, p=p, ref=o.log_prob(x, p, T), xg=o.g(zs, p, T))


def _flow_call(net, graph, dst, src, direction):
    """gnf_grevnet_from_f32: `src`'s window -> `dst`'s window (same ld: the fused kernels' out-of-place first half-step)."""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    n, d = dst.n, dst.d
    flow = net._flow(d // 2, torch.device(DEV))
    csr = csr_desc(graph, csr_of(graph), net.graph_scope())
    ws_bytes = lib.gnf_workspace_bytes(n, d, C.byref(flow))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.gnf_grevnet_from_f32(C.byref(csr), C.byref(flow), src.ptr(), src.ld, dst.ptr(), dst.ld, d, direction,
                                  _abi.ptr(sums), _abi.ptr(ws), ws_bytes, _abi.stream_ptr())
    _abi.check(rc, "gnf_grevnet_from_f32")
    torch.cuda.synchronize()
    return sums.cpu()


def _run_both(pr, layout, force_shape):
    """-> {shape: (z, sums, x_back)} for force_shape 0 and 12, on one layout; guard bands checked"""
    from gnf_amd import _abi
    n, d = pr["n"], pr["d"]
    extra, c0 = layout
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = True
    graph = graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)
    out = {}
    for shape in (0, 12):
        force_shape(shape)
        res = []
        for data, direction in ((pr["x"], _abi.GNF_FORWARD), (pr["zs"], _abi.GNF_INVERSE)):
            src = GuardBanded(n, d, d + extra, c0, device=DEV, fill=data)
            dst = GuardBanded(n, d, d + extra, c0, device=DEV)
            sums = _flow_call(net, graph, dst, src, direction)
            dst.check_guard()
            src.check_guard()
            assert torch.equal(src.window.cpu(), torch.as_tensor(data))      # the source window is read only
            res += [dst.window.cpu().clone(), sums]
        out[shape] = (res[0], res[1], res[2])
    return out


def _assert_equal_and_oracle(pr, out):
    z, sums, xb = out[0]
    z12, sums12, xb12 = out[12]
    assert torch.isfinite(z).all() and torch.isfinite(sums).all() and torch.isfinite(xb).all()
    assert torch.equal(z, z12), "z: automatic dispatch vs force_shape = 12"
    assert torch.equal(sums, sums12), f"[logdet, sum z^2]: {sums.tolist()} vs {sums12.tolist()}"
    assert torch.equal(xb, xb12), "inverse x: automatic dispatch vs force_shape = 12"
    n, d = pr["n"], pr["d"]
    lp = (-0.5 * float(sums[1]) - 0.5 * d * LN_2PI * n + float(sums[0])) / n
    err = abs(lp - pr["ref"]["log_prob_xs_per_node"])
    print(f"per-node log-prob {lp:.9g}, |delta| vs fp64 oracle {err:.3e}")
    assert err <= 1e-4
    np.testing.assert_allclose(z.numpy(), pr["ref"]["z"], atol=3e-4, rtol=3e-4)
    np.testing.assert_allclose(xb.numpy(), pr["xg"], atol=3e-4, rtol=3e-4)


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_geo_instance_bitwise_equals_generic(force_shape, gname, net):
    pr = _problem(gname, *NETS[net])
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS["contiguous"], force_shape))


@pytest.mark.parametrize("layout", ["ldD+4_c0", "ldD+3_c3"])
@pytest.mark.parametrize("gname,net", [("n47_three_graphs", "mean_leaky"), ("isolated_and_deg9to17", "sum_relu")])
def test_geo_instance_on_strided_misaligned_rows(force_shape, gname, net, layout):
    pr = _problem(gname, *NETS[net])
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS[layout], force_shape))


@pytest.mark.parametrize("geometry", ["L128_K4", "H16", "concat"])
def test_other_geometries_fall_through_to_the_generic_instance(force_shape, geometry):
    """Geometries the dispatch rule never matches: the automatic choice must reject them without error and give what
    force_shape = 12 gives."""
    kw = {"L128_K4": dict(latent=128, k=4), "H16": dict(d=32), "concat": dict(combine="concat")}[geometry]
    pr = _problem("n47_three_graphs", "mean", "leaky_relu", **kw)
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS["contiguous"], force_shape))
