"""Per-graph log-likelihoods, everything that needs no GPU: the float64 reference's own consistency, the argument
validation of gnf_grevnet_per_graph_f32 before any launch, its host-side workspace size, the no-CPU-fallback rule and the
gather helper that puts per-graph vectors of shards back into batch order (gloo, world size 2)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gnf_amd import _abi
from oracle import gnf_oracle as O

import graph_attn_ref as R
import per_graph_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(dataset, ids, d, t, seed, bn=False, **kw):
    nn, ne, s, r = O.batch_graphs(*dataset, ids)
    n = int(nn.sum())
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    p = O.make_grevnet_params(seed, d // 2, 24, 3, t, final_scale=0.4, **kw)
    if bn:
        p["bn"] = O.make_bn_params(seed + 1, d // 2, t)
    return nn, ne, s, r, n, x, p


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
def test_reference_per_graph_values_sum_to_the_batch_scalar(grid_small, community_medium, bn):
    """(a) sum_g of the per-graph values = the scalar of Fp64Dense.f, 1e-9 relative - with and without batch norm"""
    for dataset, ids in ((grid_small, list(range(12))), (community_medium, [3, 50, 7, 120])):
        nn, ne, s, r, n, x, p = _case(dataset, ids, 8, 2, 11, bn=bn)
        o = P.PerGraphDense(s, r, n)
        got = o.per_graph_terms(x, p, 2, nn)
        z, logdet = O.Fp64Dense(s, r, n).f(x, p, 2)
        np.testing.assert_array_equal(got["z"], z)
        assert abs(got["log_det_jacobian"].sum() - logdet) <= 1e-9 * max(1.0, abs(logdet))
        full = O.Fp64Dense(s, r, n).log_prob(x, p, 2)
        assert abs(got["log_prob_xs"].sum() - full["log_prob_xs"]) <= 1e-9 * abs(full["log_prob_xs"])
        assert got["num_nodes"].sum() == n


def test_reference_graph_value_equals_the_graph_run_alone(grid_small):
    """(b) additivity: without batch norm, graph g's value = Fp64Dense.f on graph g alone"""
    nn, ne, s, r, n, x, p = _case(grid_small, [0, 5, 11, 2, 7], 6, 2, 5)
    got = P.PerGraphDense(s, r, n, agg="sum").per_graph_terms(x, p, 2, nn)
    for g, (n1, e1, s1, r1, x1) in enumerate(P.single_graph_batches(nn, ne, s, r, x)):
        alone = O.Fp64Dense(s1, r1, int(n1[0]), agg="sum").log_prob(x1, p, 2)
        assert abs(got["log_det_jacobian"][g] - alone["log_det_jacobian"]) <= 1e-9 * max(1.0, abs(alone["log_det_jacobian"]))
        assert abs(got["log_prob_xs"][g] - alone["log_prob_xs"]) <= 1e-9 * abs(alone["log_prob_xs"])


def test_reference_with_batch_norm_differs_from_single_graph_runs(grid_small):
    """with batch norm the per-graph terms use the batch's moments: NOT what a graph gives alone, yet they add up"""
    nn, ne, s, r, n, x, p = _case(grid_small, [0, 5, 11, 2], 6, 2, 5, bn=True)
    got = P.PerGraphDense(s, r, n).per_graph_terms(x, p, 2, nn)
    diffs = []
    for g, (n1, e1, s1, r1, x1) in enumerate(P.single_graph_batches(nn, ne, s, r, x)):
        alone = O.Fp64Dense(s1, r1, int(n1[0])).log_prob(x1, p, 2)
        diffs.append(abs(got["log_prob_xs"][g] - alone["log_prob_xs"]))
    assert min(diffs) > 1e-3


def test_graph_attention_reference_sums_to_its_scalar():
    nn = np.array([5, 1, 9, 4])
    s, r = R.complete_edges(nn)
    n = int(nn.sum())
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, 8)).astype(np.float32)
    p = R.make_graph_attn_grevnet_params(7, 4, 16, 2, 2, num_heads=2, kq_dim=3, v_dim=5, out_dim=6)
    got = P.PerGraphGraphAttn(s, r, nn).per_graph_terms(x, p, 2)
    full = R.log_prob(nn, s, r, x, p, 2)
    assert abs(got["log_det_jacobian"].sum() - full["log_det_jacobian"]) <= 1e-9 * max(1.0, abs(full["log_det_jacobian"]))
    assert abs(got["log_prob_xs"].sum() - full["log_prob_xs"]) <= 1e-9 * abs(full["log_prob_xs"])
    # graph-scope attention never crosses a graph boundary: additivity holds for it too
    for g, (n1, e1, s1, r1, x1) in enumerate(P.single_graph_batches(nn, np.asarray(nn) ** 2, s, r, x)):
        alone = R.log_prob(n1, s1, r1, x1, p, 2)
        assert abs(got["log_prob_xs"][g] - alone["log_prob_xs"]) <= 1e-9 * abs(alone["log_prob_xs"])


def test_empty_graph_in_the_reference_gives_zero_not_nan():
    z = np.ones((3, 2))
    out = P.assemble(z, np.array([1.0, 2.0, 3.0]), 0.5, [2, 0, 1])
    assert out["log_prob_xs"][1] == 0.0 and out["log_prob_xs_per_node"][1] == 0.0
    assert out["log_det_jacobian"][0] == 3.0 + 2 * 0.5 and out["log_det_jacobian"][2] == 3.0 + 0.5


# ---- C ABI without a device ------------------------------------------------------------------------------------------
def _mlp(dims, fake_ptr=0x1000):
    m = _abi.GnfMlp()
    m.num_layers = len(dims) - 1
    for j, d in enumerate(dims):
        m.dims[j] = d
    for j in range(len(dims) - 1):
        m.W[j] = fake_ptr
        m.b[j] = fake_ptr
    return m


def _flow(t=1):
    nets = (_abi.GnfMlp * 2)(_mlp([4, 8, 4]), _mlp([4, 8, 4]))
    flow = _abi.GnfFlow(t, 1, C.cast(nets, C.POINTER(_abi.GnfMlp)), C.cast(nets, C.POINTER(_abi.GnfMlp)),
                        _abi.GnfGnnSpec(1, 0, 1.0, 1, 0.2))
    flow._keep = nets
    return flow


def _err():
    return _abi.lib().gnf_last_error().decode()


def test_per_graph_argument_validation_without_a_gpu():
    lib = _abi.lib()
    flow = _flow()
    f = lib.gnf_grevnet_per_graph_f32
    big = 1 << 24
    with_off = _abi.GnfCsr(0x1000, 0x1000, 10, 20, 0x1000, 3)
    # missing node_offsets: every GNN family needs them here
    no_off = _abi.GnfCsr(0x1000, 0x1000, 10, 20)
    assert f(C.byref(no_off), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert "node_offsets" in _err()
    no_graphs = _abi.GnfCsr(0x1000, 0x1000, 10, 20, 0x1000, 0)
    assert f(C.byref(no_graphs), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert "node_offsets" in _err()
    # odd D
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 7, 7, 0x1000, 0x1000, 0x1000, big, None) == -2
    assert "even" in _err()
    # ld < D, and a source with ld_src < D
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 4, 8, 0x1000, 0x1000, 0x1000, big, None) == -2
    # workspace too small: the plain flow workspace is not enough
    plain = lib.gnf_workspace_bytes(10, 8, C.byref(flow))
    need = lib.gnf_per_graph_workspace_bytes(10, 3, 8, C.byref(flow))
    assert need > plain
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, plain, None) == -3
    assert "workspace" in _err()
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, need - 1, None) == -3
    # graph_out == NULL, sums == NULL
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, None, 0x1000, big, None) == -1
    assert "graph_out" in _err()
    assert f(C.byref(with_off), C.byref(flow), None, 0, 0x1000, 8, 8, None, 0x1000, 0x1000, big, None) == -1
    # null flow / csr
    assert f(None, C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert f(C.byref(with_off), None, None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1


def test_per_graph_refusals_of_the_walk_without_a_gpu():
    """What the entry point checks only through the walk behind it, after its own checks (node_offsets, sums / graph_out,
    the workspace): a source with ld_src < D, a bijector without gamma / with epsilon 0, a null x - each with the code and
    the text the plain flow entry point gives."""
    lib = _abi.lib()
    f = lib.gnf_grevnet_per_graph_f32
    big = 1 << 24
    csr = _abi.GnfCsr(0x1000, 0x1000, 10, 20, 0x1000, 3)
    flow = _flow()
    assert f(C.byref(csr), C.byref(flow), 0x2000, 4, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -2
    assert _err() == "gnf_grevnet_from_f32: ld_src=4 < D=8"
    assert f(C.byref(csr), C.byref(flow), None, 0, None, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert _err() == "gnf_grevnet_f32: null x/ws"
    bns = (_abi.GnfBatchNorm * 2)()
    for q in range(2):
        bns[q].gamma, bns[q].beta, bns[q].epsilon = 0x1000, 0x1000, 1e-3
    flow.bns = C.cast(bns, C.POINTER(_abi.GnfBatchNorm))
    bns[1].gamma = None
    assert f(C.byref(csr), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert _err() == "gnf_grevnet_f32: batch-norm 1 has null gamma / beta"
    bns[1].gamma, bns[0].epsilon = 0x1000, 0.0
    assert f(C.byref(csr), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert _err() == "gnf_grevnet_f32: batch-norm 0 epsilon must be > 0"
    # the entry point's own checks come first: without node_offsets the bad bijector is not reached
    no_off = _abi.GnfCsr(0x1000, 0x1000, 10, 20)
    assert f(C.byref(no_off), C.byref(flow), None, 0, 0x1000, 8, 8, 0x1000, 0x1000, 0x1000, big, None) == -1
    assert _err().startswith("gnf_grevnet_per_graph_f32: needs GnfCsr.node_offsets")
    # ... and so does the empty batch's early return
    empty = _abi.GnfCsr(0, 0, 0, 0)
    assert f(C.byref(empty), C.byref(flow), None, 0, None, 8, 8, 0x1000, None, None, 0, None) == 0


def test_per_graph_empty_batch_is_a_no_op_success():
    """no nodes and no graphs: GNF_OK after validation, without touching a device"""
    lib = _abi.lib()
    flow = _flow()
    csr = _abi.GnfCsr(0, 0, 0, 0)
    assert lib.gnf_grevnet_per_graph_f32(C.byref(csr), C.byref(flow), None, 0, None, 8, 8, 0x1000, None, None, 0, None) == 0
    # ... but still validated
    assert lib.gnf_grevnet_per_graph_f32(C.byref(csr), C.byref(flow), None, 0, None, 7, 7, 0x1000, None, None, 0, None) == -2


def test_per_graph_workspace_is_a_monotone_host_computation():
    lib = _abi.lib()
    flow = _flow(t=3)
    w = lib.gnf_per_graph_workspace_bytes
    sizes = [w(n, 4, 8, C.byref(flow)) for n in (0, 1, 10, 100, 1000, 5000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    by_graphs = [w(100, b, 8, C.byref(flow)) for b in (1, 2, 50, 100)]
    assert all(a <= b for a, b in zip(by_graphs, by_graphs[1:]))
    # the flow's own workspace + 2T slots of one double per node + 2T bijector terms
    assert w(100, 4, 8, C.byref(flow)) >= lib.gnf_workspace_bytes(100, 8, C.byref(flow)) + 6 * 101 * 8
    assert w(100, 4, 8, None) == 0 and w(-1, 4, 8, C.byref(flow)) == 0 and w(100, -1, 8, C.byref(flow)) == 0


def test_abi_version_unchanged_by_the_new_entry_points():
    assert _abi.lib().gnf_abi_version() == 10 and _abi.GNF_ABI_VERSION == 10
    assert "gnf_grevnet_per_graph_f32" in _abi.EXPORTED_SYMBOLS and "gnf_per_graph_workspace_bytes" in _abi.EXPORTED_SYMBOLS


def test_per_graph_fails_loudly_without_a_hip_device():
    from helpers import graph_from_arrays, make_product_grevnet
    from gnf_amd.flow import log_prob_per_graph
    hp = dict(D=4, latent=8, K=2, T=1, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu",
              weight_sharing=False)
    net = make_product_grevnet(hp, None)
    g = graph_from_arrays([2], [2], [0, 1], [0, 1], np.zeros((2, 4), np.float32))
    with pytest.raises(_abi.GnfError):
        net.f_per_graph(g)
    with pytest.raises(_abi.GnfError):
        net.log_prob_per_graph(g)
    with pytest.raises(_abi.GnfError):
        log_prob_per_graph(net, g)


# ---- gather helper -----------------------------------------------------------------------------------------------------
def test_gather_per_graph_single_process_is_the_permutation():
    from gnf_amd.sharding import gather_per_graph
    ids = [np.array([2, 0, 3, 1])]
    v = torch.tensor([20.0, 0.0, 30.0, 10.0], dtype=torch.float64)
    assert gather_per_graph(v, ids).tolist() == [0.0, 10.0, 20.0, 30.0]
    with pytest.raises(ValueError):
        gather_per_graph(v[:3], ids)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, ret):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gnf_amd.sharding import gather_per_graph, shard_graph_ids
        d = np.load(os.path.join(ROOT, "data", "community_medium.npz"))
        rng = np.random.default_rng(4)
        ids = rng.choice(168, size=9, replace=True)
        shards = shard_graph_ids(d["n_node"][ids], d["n_edge"][ids], world)
        mine = shards[rank]
        local = torch.as_tensor(100.0 * mine + 0.5, dtype=torch.float64)          # a value that names its graph
        got = gather_per_graph(local, shards)
        two = gather_per_graph(torch.stack([local, -local], dim=1), shards)
        ret[rank] = (got.tolist(), two.tolist(), [len(s) for s in shards])
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gather_per_graph_gloo_world_size_2():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_gather_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert len(ret) == world
    want = [100.0 * g + 0.5 for g in range(9)]
    for rank in range(world):
        got, two, sizes = ret[rank]
        assert sum(sizes) == 9 and sizes[0] != 0 and sizes[1] != 0
        assert got == want
        assert [row[0] for row in two] == want and [row[1] for row in two] == [-v for v in want]
