"""Graph-scope attention (MultiheadSelfAttention / SelfAttention, GnfAttn.scope == GNF_ATTN_GRAPH) without a GPU: the
float64 restatement against the reference's literal op order and against finite differences, and the C ABI's argument
validation on fake pointers (every rejection happens before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_attn_ref as R
from gnf_amd import _abi

N_NODE = np.array([1, 7, 3, 12, 5])   # unequal sizes, one graph of a single node


@pytest.mark.parametrize("heads,kq,v,div", [(3, 4, 5, True), (1, 6, 6, False), (8, 10, 10, True)])
def test_restatement_equals_the_literal_masked_batch_softmax(heads, kq, v, div):
    rng = np.random.default_rng(heads * 100 + kq)
    h = 6
    x = rng.standard_normal((int(N_NODE.sum()), h))
    a = R.make_graph_attn_net_params(rng, h, 8, 2, num_heads=heads, kq_dim=kq, v_dim=v, out_dim=5,
                                     kq_dim_division=div, dtype=np.float64)["attn"]
    s, r = R.complete_edges(N_NODE)
    o = R.GraphAttnGather(s, r, N_NODE)
    pa = o.prep_params({"s": [{"attn": a, "mlp": []}]})["s"][0]["attn"]
    got = o.attended(o.to_t(x), pa).numpy()
    want = R.literal_attended(x, a, N_NODE)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # the single-node graph attends to itself only
    np.testing.assert_allclose(got[0], (x[0] @ a["wv"]), rtol=0, atol=1e-12)


N_NODE_EMPTIES = np.array([0, 3, 1, 0, 0, 6, 1, 1, 4, 0])   # empty graphs leading, interior (in a row), trailing


@pytest.mark.parametrize("heads,kq,v,div", [(3, 4, 5, True), (1, 6, 6, False)])
def test_per_graph_form_equals_the_dense_form_and_the_literal(heads, kq, v, div):
    """The per-graph oracle (GraphAttnGather(per_graph=True), O(sum n_g^2)) against the dense [heads, N, N] form and the
    reference's literal op order, forward and float64 autograd gradients of a whole flow, on a batch with empty and one-node
    graphs."""
    rng = np.random.default_rng(heads * 10 + kq)
    h = 5
    n = int(N_NODE_EMPTIES.sum())
    x = rng.standard_normal((n, h))
    a = R.make_graph_attn_net_params(rng, h, 8, 2, num_heads=heads, kq_dim=kq, v_dim=v, out_dim=4 if heads > 1 else None,
                                     kq_dim_division=div, dtype=np.float64)["attn"]
    s, r = np.zeros(0, np.int32), np.zeros(0, np.int32)
    outs = []
    for per_graph in (False, True):
        o = R.GraphAttnGather(s, r, N_NODE_EMPTIES, per_graph=per_graph)
        pa = o.prep_params({"s": [{"attn": a, "mlp": []}]})["s"][0]["attn"]
        outs.append(o.attended(o.to_t(x), pa).numpy())
    np.testing.assert_allclose(outs[1], outs[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(outs[1], R.literal_attended(x, a, N_NODE_EMPTIES), rtol=0, atol=1e-12)
    for i in np.cumsum(N_NODE_EMPTIES)[N_NODE_EMPTIES == 1] - 1:       # one-node graphs: exactly their own v
        np.testing.assert_allclose(outs[1][i], x[i] @ a["wv"], rtol=0, atol=1e-14)
    # a whole flow: log-prob, z, inverse and every gradient
    d, t = 6, 2
    kw = dict(num_heads=heads, kq_dim=kq, v_dim=v, kq_dim_division=div)
    if heads > 1:
        kw.update(out_dim=4, layer_norm=True)
    p = R.make_graph_attn_grevnet_params(21, d // 2, 8, 2, t, dtype=np.float64, final_scale=0.25, **kw)
    x = rng.standard_normal((n, d))
    dense, per = (R.loss_and_grads(N_NODE_EMPTIES, s, r, x, p, t, activation="relu", per_graph=pg) for pg in (False, True))
    assert abs(per["total_loss"] - dense["total_loss"]) <= 1e-10 * max(1.0, abs(dense["total_loss"]))
    np.testing.assert_allclose(per["z"], dense["z"], rtol=1e-12, atol=1e-12)
    for gp, gd in zip(_flat(per["grads"]), _flat(dense["grads"])):
        np.testing.assert_allclose(gp, gd, rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(R.inverse(N_NODE_EMPTIES, s, r, per["z"], p, t, activation="relu", per_graph=True), x,
                               rtol=0, atol=1e-10)


def _flat(g):
    out = []
    if isinstance(g, dict):
        for k in sorted(g):
            out += _flat(g[k])
    elif isinstance(g, (list, tuple)):
        for q in g:
            out += _flat(q)
    else:
        out.append(g)
    return out


@pytest.mark.parametrize("kind", ["multihead_ln", "single"])
def test_restatement_gradients_match_central_differences(kind):
    """Every weight kind (wq, wk, wv, wo, ln_gamma, ln_beta, the MLP) of a T = 1 flow with batch norm."""
    rng = np.random.default_rng(7)
    n_node = np.array([1, 4, 3])
    n, d = int(n_node.sum()), 4
    kw = dict(num_heads=2, kq_dim=3, v_dim=2, out_dim=3, layer_norm=True) if kind == "multihead_ln" else \
        dict(num_heads=1, kq_dim=3, v_dim=2)
    p = R.make_graph_attn_grevnet_params(11, d // 2, 6, 2, 1, dtype=np.float64, **kw)
    from oracle import gnf_oracle as O
    p["bn"] = [[{k: (np.asarray(v, np.float64) if k != "epsilon" else v) for k, v in b.items()} for b in half]
               for half in O.make_bn_params(12, d // 2, 1)]
    x = rng.standard_normal((n, d))
    s, r = np.zeros(0, np.int32), np.zeros(0, np.int32)     # the edges play no part
    ref = R.loss_and_grads(n_node, s, r, x, p, 1, activation="relu")
    # perturb scalars of every tensor in place (the grads share the layout of p)
    params_flat, grads_flat = [], []

    def collect(m, g):
        if isinstance(m, dict) and "attn" in m:
            for k in R.graph_attn_weight_keys(m["attn"]):
                params_flat.append(m["attn"][k])
                grads_flat.append(g["attn"][k])
            collect(m["mlp"], g["mlp"])
        elif isinstance(m, dict) and "gamma" in m:
            params_flat.extend([m["gamma"], m["beta"]])
            grads_flat.extend([g["gamma"], g["beta"]])
        elif isinstance(m, list) and m and isinstance(m[0], tuple):
            for (w, b), (gw, gb) in zip(m, g):
                params_flat.extend([w, b])
                grads_flat.extend([gw, gb])
        elif isinstance(m, list):
            for q, gq in zip(m, g):
                collect(q, gq)
    for key in ("s", "t", "bn"):
        collect(p[key], ref["grads"][key])
    n_attn = 6 if kind == "multihead_ln" else 3
    assert len(params_flat) == 4 * (n_attn + 4) + 4
    eps = 1e-6
    for w, g in zip(params_flat, grads_flat):
        assert w.dtype == np.float64
        for idx in list(np.ndindex(w.shape))[:6]:
            old = w[idx]
            w[idx] = old + eps
            lp = R.loss_and_grads(n_node, s, r, x, p, 1, activation="relu")["total_loss"]
            w[idx] = old - eps
            lm = R.loss_and_grads(n_node, s, r, x, p, 1, activation="relu")["total_loss"]
            w[idx] = old
            fd = (lp - lm) / (2 * eps)
            assert abs(fd - g[idx]) <= 1e-6 * max(1.0, abs(fd)), (w.shape, idx, fd, g[idx])


# ---- C ABI on fake pointers ------------------------------------------------------------------------------------------
FAKE = 0x1000


def _mlp(dims):
    m = _abi.GnfMlp()
    m.num_layers = len(dims) - 1
    for j, d in enumerate(dims):
        m.dims[j] = d
    for j in range(len(dims) - 1):
        m.W[j] = FAKE
        m.b[j] = FAKE
    return m


def _attn(heads=8, kq=10, v=10, out=80, wo=True, scope=_abi.GNF_ATTN_GRAPH, concat=1, residual=0):
    return _abi.GnfAttn(heads, kq, v, out, concat, 1, residual, 0, FAKE, FAKE, FAKE, FAKE if wo else 0, 0, 0, scope)


def _call(s_attn, t_attn=None, n=10, offsets=FAKE, n_graphs=2, h=1):
    """gnf_grevnet_f32 (forward) on fake pointers; returns (code, message)"""
    lib = _abi.lib()
    t_attn = t_attn if t_attn is not None else s_attn
    dims = [h + s_attn.out_dim, 16, h]
    nets_s = (_abi.GnfMlp * 2)(_mlp(dims), _mlp(dims))
    nets_t = (_abi.GnfMlp * 2)(_mlp(dims), _mlp(dims))
    keep = [s_attn, t_attn]
    for q in range(2):
        nets_s[q].attn = C.pointer(s_attn)
        nets_t[q].attn = C.pointer(t_attn)
    flow = _abi.GnfFlow(1, 1, C.cast(nets_s, C.POINTER(_abi.GnfMlp)), C.cast(nets_t, C.POINTER(_abi.GnfMlp)),
                        _abi.GnfGnnSpec(0, 0, 0.0, 0, 0.0))
    csr = _abi.GnfCsr(FAKE, FAKE, n, 4 * n, offsets, n_graphs)
    # (an empty batch: the inverse direction, which writes no sums, so nothing touches a device)
    rc = lib.gnf_grevnet_f32(C.byref(csr), C.byref(flow), FAKE, 2 * h, 2 * h, 0 if n else 1, FAKE if n else None, FAKE,
                             1 << 40, None)
    del keep
    return rc, lib.gnf_last_error().decode()


def test_abi_v10_layout():
    assert _abi.GNF_ABI_VERSION == 10 and _abi.lib().gnf_abi_version() == 10
    # fields appended at the end: positional constructors of v9 still fill the same leading fields
    assert [f[0] for f in _abi.GnfCsr._fields_][-2:] == ["node_offsets", "n_graphs"]
    assert _abi.GnfAttn._fields_[-1][0] == "scope"
    assert _abi.GnfCsr(1, 2, 3, 4).node_offsets is None and _abi.GnfAttn().scope == _abi.GNF_ATTN_EDGES


def test_graph_scope_needs_node_offsets():
    rc, msg = _call(_attn(), offsets=0)
    assert rc == -1 and "node_offsets" in msg
    rc, msg = _call(_attn(), n_graphs=0)
    assert rc == -1 and "node_offsets" in msg


def test_graph_scope_concat_and_residual_are_fixed():
    assert _call(_attn(concat=0))[0] == -1
    assert _call(_attn(residual=1))[0] == -1


def test_unknown_scope_is_rejected():
    rc, msg = _call(_attn(scope=2))
    assert rc == -1 and "scope" in msg


def test_no_output_projection_needs_one_head_of_out_dim_v():
    assert _call(_attn(heads=2, kq=4, v=4, out=8, wo=False))[0] == -2
    assert _call(_attn(heads=1, kq=4, v=4, out=5, wo=False))[0] == -2


@pytest.mark.parametrize("heads,kq,v", [(65, 1, 1), (8, 33, 10), (8, 10, 33), (1, 257, 4), (1, 4, 257)])
def test_graph_scope_geometry_limit(heads, kq, v):
    rc, msg = _call(_attn(heads=heads, kq=kq, v=v, out=8))
    assert rc == -2 and "graph-scope" in msg


def test_s_and_t_nets_of_different_scope_are_rejected():
    rc, _ = _call(_attn(), _attn(scope=_abi.GNF_ATTN_EDGES))
    assert rc < 0


def test_empty_batch_is_ok():
    assert _call(_attn(), n=0, offsets=0, n_graphs=0)[0] == 0
    assert _call(_attn(heads=1, kq=64, v=64, out=64, wo=False), n=0, h=100)[0] == 0


def test_graph_scope_declines_the_attention_stash():
    lib = _abi.lib()
    for at in (_attn(), _attn(heads=1, kq=64, v=64, out=64, wo=False)):
        dims = [1 + at.out_dim, 16, 1]
        nets = (_abi.GnfMlp * 2)(_mlp(dims), _mlp(dims))
        for q in range(2):
            nets[q].attn = C.pointer(at)
        flow = _abi.GnfFlow(3, 1, C.cast(nets, C.POINTER(_abi.GnfMlp)), C.cast(nets, C.POINTER(_abi.GnfMlp)),
                            _abi.GnfGnnSpec(0, 0, 0.0, 0, 0.0))
        assert lib.gnf_attn_stash_bytes(100, 2, C.byref(flow)) == 0
        assert lib.gnf_workspace_bytes(100, 2, C.byref(flow)) > 0
        assert lib.gnf_backward_workspace_bytes(100, 2, C.byref(flow)) > 0


def test_factories_select_the_graph_scope_classes():
    from gnf_amd import gnn
    from gnf_amd.factories import make_gnn_fn
    base = dict(D=2, latent=16, K=2, T=1, activation="relu", weight_sharing=False)
    b = make_gnn_fn(dict(base, attn=dict(scope="graph", kq_dim=10, v_dim=10, num_heads=8, out_dim=80)))()
    assert type(b) is gnn.MultiheadSelfAttention and b.kq_dim_division and b.attn_keys() == ("wq", "wk", "wv", "wo")
    b = make_gnn_fn(dict(base, attn=dict(scope="graph", kq_dim=64, v_dim=64)))()
    assert type(b) is gnn.SelfAttention and b.in_dim(100) == 164 and b.attn_keys() == ("wq", "wk", "wv")
    b.ensure_attn_built(3, "cpu")
    assert tuple(b.attn_params["wv"].shape) == (3, 64)
    m = gnn.multihead_self_attn_gnn(4, 5, 7, lambda: gnn.MLP([8, 2]), num_heads=3, layer_norm=True)
    m.ensure_attn_built(2, "cpu")
    assert {k: tuple(v.shape) for k, v in m.attn_params.items()} == \
        {"wq": (2, 12), "wk": (2, 12), "wv": (2, 15), "wo": (15, 7), "ln_gamma": (2,), "ln_beta": (2,)}
    lim = np.sqrt(6.0 / (15 + 7))          # xavier-uniform, Wo included
    assert float(m.attn_params["wo"].abs().max()) <= lim
    assert float(m.attn_params["wo"].std()) > 0.3 * lim


def test_node_offsets_are_the_exclusive_prefix_sum():
    from gnf_amd.graphs import GraphsTuple, node_offsets_of
    g = GraphsTuple(nodes=torch.zeros(10, 2), edges=None, receivers=torch.zeros(0, dtype=torch.int32),
                    senders=torch.zeros(0, dtype=torch.int32), globals=None,
                    n_node=torch.tensor([3, 0, 7], dtype=torch.int32), n_edge=torch.zeros(3, dtype=torch.int32))
    assert node_offsets_of(g).tolist() == [0, 3, 3, 10]
