"""Per-graph likelihood of generated graphs, the parts that need no GPU: the ABI surface of include/gnf_inverse_per_graph.h
and the float64 reference of tests/inverse_per_graph_ref.py against a brute-force Jacobian of the oracle's Fp64Dense.g."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import inverse_per_graph_ref as IP
from oracle import gnf_oracle as O
from timestep_gnn_ref import ring_chord_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))


# ---- ABI surface -----------------------------------------------------------------------------------------------------
def test_every_prototype_of_the_new_header_is_exported_listed_and_bound():
    from gnf_amd import _abi
    lib = _abi.lib()
    syms = _declared("gnf_inverse_per_graph.h")
    assert "gnf_grevnet_inverse_per_graph_f32" in syms and "gnf_inverse_per_graph_workspace_bytes" in syms
    assert sorted(_abi.INVERSE_PER_GRAPH_SYMBOLS) == syms
    for s in syms:
        fn = getattr(lib, s)   # AttributeError: declared, not exported
        assert fn.argtypes is not None and fn.restype is not None, s
    # gnf.h gained the include line only: its own prototype list is still EXPORTED_SYMBOLS
    assert sorted(_abi.EXPORTED_SYMBOLS) == _declared("gnf.h")
    assert '#include "gnf_inverse_per_graph.h"' in open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert not set(_abi.INVERSE_PER_GRAPH_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS)
    assert lib.gnf_abi_version() == 10
    # enum GnfRoute and the binding's names agree
    text = open(os.path.join(ROOT, "include", "gnf_inverse_per_graph.h")).read()
    enum = re.findall(r"GNF_ROUTE_([A-Z0-9_]+) = 1 << (\d+)", text)
    assert {name.lower(): 1 << int(k) for name, k in enum} == _abi.ROUTE_BITS


def _mlp(dims, fake_ptr=0x1000):
    from gnf_amd import _abi
    m = _abi.GnfMlp()
    m.num_layers = len(dims) - 1
    for j, d in enumerate(dims):
        m.dims[j] = d
    for j in range(len(dims) - 1):
        m.W[j] = fake_ptr
        m.b[j] = fake_ptr
    return m


def test_workspace_is_monotone_and_at_least_the_plain_one():
    from gnf_amd import _abi
    lib = _abi.lib()
    s = (_abi.GnfMlp * 2)(_mlp([8, 32, 8]), _mlp([8, 32, 8]))
    flow = _abi.GnfFlow(3, 1, C.cast(s, C.POINTER(_abi.GnfMlp)), C.cast(s, C.POINTER(_abi.GnfMlp)), _abi.GnfGnnSpec(1, 0, 1.0, 1, 0.2))
    f = lib.gnf_inverse_per_graph_workspace_bytes
    sizes = [f(n, 4, 16, C.byref(flow)) for n in (0, 1, 16, 17, 100, 1000, 78000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1]
    by_graphs = [f(1000, b, 16, C.byref(flow)) for b in (1, 2, 64, 1000)]
    assert all(a <= b for a, b in zip(by_graphs, by_graphs[1:]))
    for n in (0, 1, 17, 1000):
        plain = lib.gnf_workspace_bytes(n, 16, C.byref(flow))
        got = f(n, 4, 16, C.byref(flow))
        # the plain workspace (256-aligned), 2T x n row sums and 2T bijector terms, all fp64
        assert got == (plain + 255) // 256 * 256 + (6 * n + 6) * 8 and got >= plain
    assert f(-1, 4, 16, C.byref(flow)) == 0 and f(10, -1, 16, C.byref(flow)) == 0 and f(10, 4, 16, None) == 0


def test_argument_checks_that_need_no_device():
    from gnf_amd import _abi
    lib = _abi.lib()
    s = (_abi.GnfMlp * 2)(_mlp([8, 32, 8]), _mlp([8, 32, 8]))
    flow = _abi.GnfFlow(1, 1, C.cast(s, C.POINTER(_abi.GnfMlp)), C.cast(s, C.POINTER(_abi.GnfMlp)), _abi.GnfGnnSpec(1, 0, 1.0, 1, 0.2))
    csr = _abi.GnfCsr()
    csr.n_nodes, csr.n_edges, csr.n_graphs = 0, 0, 2     # graphs without their boundaries
    fn = lib.gnf_grevnet_inverse_per_graph_f32
    assert fn(C.byref(csr), C.byref(flow), None, 16, None, 16, 16, C.c_void_p(8), C.c_void_p(8), None, 0, None) == -1
    assert "node_offsets" in lib.gnf_last_error().decode()
    csr.n_graphs = 0                                      # nothing at all: only sums is needed
    assert fn(C.byref(csr), C.byref(flow), None, 16, None, 16, 16, None, None, None, 0, None) == -1
    assert "sums" in lib.gnf_last_error().decode()
    assert lib.gnf_last_route() == 0


# ---- the reference against a brute-force Jacobian -------------------------------------------------------------------------
SIZES = [1, 3, 0, 5, 2]
D, T, H_STEP = 4, 2, 1e-6


def _jacobian(fn, z):
    n, d = z.shape
    jac = np.zeros((n * d, n * d))
    for k in range(n * d):
        e = np.zeros(n * d)
        e[k] = H_STEP
        jac[:, k] = ((fn(z + e.reshape(n, d)) - fn(z - e.reshape(n, d))) / (2 * H_STEP)).ravel()
    return jac


def _case(kind, bn):
    nn, ne, s, r = ring_chord_batch(SIZES, edgeless=())
    n = int(nn.sum())
    rng = np.random.default_rng(5 + len(kind) + (3 if bn else 0))
    z = rng.standard_normal((n, D))
    if kind == "edge_attn":
        akw = dict(num_heads=2, kq_dim=3, v_dim=3, out_dim=6, concat=True, kq_dim_division=True, residual=False)
        p = O.make_attn_grevnet_params(11, D // 2, 8, 2, T, weight_sharing=False, final_scale=0.3, **akw)
        kw = dict(agg="mean", combine="agg", epsilon=0.0, activation="relu")
    else:
        agg, combine = kind.split("_")
        p = O.make_grevnet_params(7, D // 2, 8, 2, T, combine=combine, final_scale=0.3)
        kw = dict(agg=agg, combine=combine, epsilon=0.5 if combine == "agg" else 0.0, activation="leaky_relu")
    if bn:
        p["bn"] = O.make_bn_params(9, D // 2, T)
    return nn, s, r, z, p, kw


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("kind", ["mean_agg", "sum_concat", "edge_attn"])
def test_reference_equals_the_block_slogdet_of_a_brute_force_jacobian(kind, bn):
    nn, s, r, z, p, kw = _case(kind, bn)
    n = int(nn.sum())
    ref_net = IP.InversePerGraphDense(s, r, n, **kw)
    ref = ref_net.per_graph_terms(z, p, T, nn)
    np.testing.assert_array_equal(ref["x"], O.Fp64Dense(s, r, n, **kw).g(z, p, T))   # the same loop
    jac = _jacobian(lambda v: O.Fp64Dense(s, r, n, **kw).g(v, p, T), z)
    off = np.concatenate([[0], np.cumsum(nn)]) * D
    worst = 0.0
    for a in range(len(nn)):
        for b in range(len(nn)):
            blk = jac[off[a]:off[a + 1], off[b]:off[b + 1]]
            if a != b:
                assert not blk.any(), (a, b)   # exactly 0: g never mixes graphs, with or without batch norm
            elif nn[a] == 0:
                assert ref["log_det_jacobian"][a] == 0.0
            else:
                sign, logabs = np.linalg.slogdet(blk)
                assert sign != 0
                worst = max(worst, abs(logabs - ref["log_det_jacobian"][a]))
    print(f"[inverse-per-graph] {kind} bn={bn}: worst |slogdet - reference| over the graphs {worst:.3e}")
    assert worst <= 1e-7
    # the gather formulation keeps the same books
    gat = IP.InversePerGraphGather(s, r, nn, **kw).per_graph_terms(z, p, T)
    np.testing.assert_allclose(gat["log_det_jacobian"], ref["log_det_jacobian"], atol=1e-10)
    np.testing.assert_allclose(gat["x"], ref["x"], atol=1e-10)
    if not bn:   # f inverts g exactly, so its log-det at g(z) is minus the total
        _, logdet_f = O.Fp64Dense(s, r, n, **kw).f(ref["x"], p, T)
        assert abs(logdet_f + ref["log_det_jacobian"].sum()) <= 1e-12


def _seed_cases():
    import inverse_per_graph_cases as IC
    return IC.all_cases()


@pytest.mark.parametrize("case", _seed_cases(), ids=[c[0] for c in _seed_cases()])
def test_device_cases_leave_the_cpu_restatements_inside_half_the_bounds(case):
    """the seeds of tests/inverse_per_graph_cases.py: the float64 restatements (dense and gather) agree, and the float32 one
    stays within HALF of the device tests' per-node bound and of their bound on x - so a failure there is the device's"""
    import torch
    import inverse_per_graph_cases as IC
    name, build, kind = case
    hp, nn, ne, s, r, z, p = build()
    g64 = IC.gather_ref(hp, nn, s, r, z, p)
    ref = g64 if kind == "gather" else IC.dense_ref(hp, nn, s, r, z, p)
    e64 = IC.per_node_errors(g64, ref, nn)
    r32 = IC.gather_ref(hp, nn, s, r, z, p, dtype=torch.float32)
    e32 = IC.per_node_errors(r32, ref, nn)
    tol = IC.ln_tol(hp, nn, s, r, z, p, ref) if kind == "ln" else IC.TOL
    x_excess = float((np.abs(r32["x"] - ref["x"]) / (IC.X_TOL * (1.0 + np.abs(ref["x"])))).max())
    print(f"[inverse-per-graph] {name}: fp64 gather vs reference {max(e64.values()):.2e}, fp32 {max(e32.values()):.2e} of {tol:.2e}; "
          f"x at {x_excess:.2f} of its bound; max |x| {np.abs(ref['x']).max():.2f}")
    assert np.isfinite(ref["x"]).all() and np.isfinite(ref["log_det_jacobian"]).all()
    assert max(e64.values()) <= 1e-9
    assert 2.0 * max(e32.values()) <= tol, e32
    assert 2.0 * x_excess <= 1.0, x_excess


def test_assemble_adds_up_and_gives_zero_for_an_empty_graph():
    nn, s, r, z, p, kw = _case("mean_agg", True)
    ref = IP.InversePerGraphDense(s, r, int(nn.sum()), **kw).per_graph_terms(z, p, T, nn)
    assert ref["log_prob_xs"][2] == 0.0 and ref["log_prob_xs_per_node"][2] == 0.0 and ref["sumsq"][2] == 0.0
    np.testing.assert_allclose(ref["log_prob_xs"], ref["log_prob_zs"] - ref["log_det_jacobian"], rtol=0, atol=0)
    assert abs(ref["sumsq"].sum() - float((z * z).sum())) <= 1e-12
    want_c = sum(IP.bn_term(b) for half in p["bn"] for b in half)
    assert abs(ref["c_total"] - want_c) <= 1e-13
