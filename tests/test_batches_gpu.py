"""Batch assembly on the device (include/gnf_batches.h, datasets.DeviceGraphDataset / complete_batch): every output integer
for integer against tests/batches_ref.py AND against the parent route run on the device (upload, build_csr_device twice);
guard bands around every output, at every 16-byte misalignment; an out-of-range id and sizes that do not match the ids
through the raw entry point; the paths the launch takes (offsets in LDS / in global memory, one / four groups per thread);
then the consumers - the flow and the encoder's trainer see the same batch bit for bit - the chunk readers on a device, and
both example drivers with --device_batches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batches_ref as R
from gnf_amd import _abi, datasets as D, graphs
from gnf_amd.graphs import build_csr_device, csr_of, graphs_tuple_from_edge_lists, node_offsets_of
from helpers import graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5EEDBA5E


@pytest.fixture(autouse=True)
def _leave_the_process_wide_generators_as_found():
    """Networks built here draw their initial weights from gnn._GEN, one stream for the whole process, and torch.randn from
    torch's: tests that run later in the same process build their nets from whatever state they find (the self_attn case of
    tests/test_param_arena_gpu.py went to NaN on the weights it drew behind this module), so every test here puts both back."""
    from gnf_amd import gnn
    kept = gnn._GEN.get_state(), torch.random.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    gnn._GEN.set_state(kept[0])
    torch.random.set_rng_state(kept[1])
    torch.cuda.set_rng_state(kept[2], DEV)


@pytest.fixture(scope="module")
def host_ds():
    return R.dataset()


@pytest.fixture(scope="module")
def dev_ds(host_ds):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return D.DeviceGraphDataset(host_ds, 4, device=DEV)


def _t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _graph_outputs(g):
    """the ten outputs as batch_of / complete_batch hand them over: the GraphsTuple's fields and the seeded caches"""
    csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
    e = int(g.senders.shape[0])
    return dict(n_node=g.n_node, n_edge=g.n_edge, node_offsets=node_offsets_of(g), senders=g.senders, receivers=g.receivers,
                rowptr=csr.rowptr, col=csr.col[:e], rowptr_t=csr_t.rowptr, col_t=csr_t.col[:e])


def _no_build(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("gnf_build_csr ran: the CSR cache was not seeded")
    monkeypatch.setattr(graphs, "build_csr_device", refuse)


class Guarded:
    """int32 [n] outputs, each inside a buffer of sentinels with `lead` words in front (lead % 4 = the 16-byte misalignment)"""

    def __init__(self, sizes, leads, tail=19):
        self.bufs, self.views = [], []
        for n, lead in zip(sizes, leads):
            buf = torch.full((lead + n + tail,), SENTINEL, dtype=torch.int32, device=DEV)
            self.bufs.append((buf, lead, n))
            self.views.append(buf[lead:lead + n])

    def ptrs(self):
        return [C.c_void_p(v.data_ptr()) for v in self.views]

    def check(self):
        for k, (buf, lead, n) in enumerate(self.bufs):
            assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all()), f"guard of output {k} changed"


def _raw_assemble(dev_ds, ids, n, e, leads):
    b = len(ids)
    out = Guarded([b, b, b + 1, e, e, n + 1, e, n + 1, e], leads)
    lib = _abi.lib()
    ws_bytes = lib.gnf_batch_assemble_workspace_bytes(b)
    ws = Guarded([(ws_bytes + 3) // 4], [64])
    gid = _t(np.asarray(ids, np.int32))
    _abi.check(lib.gnf_batch_assemble(C.byref(dev_ds._store), _abi.ptr(gid), b, n, e, *out.ptrs(), ws.ptrs()[0], ws_bytes,
                                      _abi.stream_ptr(torch.device(DEV))), "gnf_batch_assemble")
    torch.cuda.synchronize()
    out.check()
    ws.check()
    return dict(zip(R.ASSEMBLE_KEYS, out.views))


# ---- gnf_batch_assemble ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "one", "mixed", "reversed", "drawn64"])
def test_batch_of_equals_the_reference_and_the_parent_route(host_ds, dev_ds, name, monkeypatch):
    ids = R.id_lists(host_ds)[name]
    want = R.host_route(host_ds, ids)
    n = int(want["node_offsets"][-1])
    x = torch.zeros(n, 4, device=DEV)
    # the parent route on the device: host assembly, upload, gnf_build_csr twice
    parent = graphs_tuple_from_edge_lists(host_ds.n_node, host_ds.n_edge, host_ds.senders, host_ds.receivers, ids,
                                          np.zeros((n, 4), np.float32), DEV)
    e = int(parent.senders.shape[0])
    pc, pt = build_csr_device(parent), build_csr_device(parent, by_sender=True)
    parent_out = dict(n_node=parent.n_node, n_edge=parent.n_edge, senders=parent.senders, receivers=parent.receivers,
                      rowptr=pc.rowptr, col=pc.col[:e], rowptr_t=pt.rowptr, col_t=pt.col[:e])
    _no_build(monkeypatch)
    g = dev_ds.batch_of(ids, nodes=x)
    got = _graph_outputs(g)
    torch.cuda.synchronize()
    assert g.nodes.data_ptr() == x.data_ptr() and g.edges.shape == (e,) and g.globals.shape == (len(ids),)
    for k in R.ASSEMBLE_KEYS:
        assert got[k].dtype == torch.int32 and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
        if k in parent_out:
            assert torch.equal(got[k], parent_out[k].to(torch.int32)), k
    # two calls give the same bits (the second draws its features)
    again = _graph_outputs(dev_ds.batch_of(ids))
    assert all(torch.equal(again[k], got[k]) for k in R.ASSEMBLE_KEYS)


@pytest.mark.parametrize("name", ["empty", "one", "mixed", "reversed", "drawn64"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_raw_entry_point_leaves_guard_bands_untouched_at_every_misalignment(host_ds, dev_ds, name, shift):
    ids = R.id_lists(host_ds)[name]
    want = R.host_route(host_ds, ids)
    n, e = int(want["node_offsets"][-1]), len(want["senders"])
    got = _raw_assemble(dev_ds, ids, n, e, [16 + (shift + k) % 4 for k in range(9)])
    if len(ids) == 0:          # n_batch == 0: rowptr[0] = rowptr_t[0] = 0 and nothing else
        assert got["rowptr"].tolist() == [0] and got["rowptr_t"].tolist() == [0] and got["node_offsets"].tolist() == [SENTINEL]
        return
    for k in R.ASSEMBLE_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k


def test_out_of_range_ids_and_sizes_that_do_not_match_stay_inside_the_arrays(host_ds, dev_ds):
    g = len(host_ds)
    ids = [3, g, -5, 2, 2 ** 31 - 1, -2 ** 31, 6]
    clamped = [min(max(i, 0), g - 1) for i in ids]
    want = R.host_route(host_ds, clamped)
    n, e = int(want["node_offsets"][-1]), len(want["senders"])
    got = _raw_assemble(dev_ds, ids, n, e, [17] * 9)                 # clamped into range: the clamped batch, guards intact
    for k in R.ASSEMBLE_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    # N and E smaller and larger than the ids' sums: wrong numbers, and still every guard intact (checked inside)
    _raw_assemble(dev_ds, ids, n - 7, e - 1001, [18] * 9)
    _raw_assemble(dev_ds, ids, n + 5, e + 3000, [19] * 9)
    _raw_assemble(dev_ds, [R.EDGELESS, R.EDGELESS], 8, 0, [16] * 9)  # a batch without edges: no edge job at all


def test_offsets_in_global_memory_and_four_groups_per_thread(host_ds, dev_ds, monkeypatch):
    """4100 slots: the offsets no longer fit the LDS copy (GNF_BATCH_LDS_SLOTS = 4095), and more than 2^20 output words: four
    groups per thread.  The reference is the cut-and-rebase statement (tests/test_batches_cpu.py holds it to the host route)."""
    ids = np.random.default_rng(4100).integers(0, len(host_ds), size=4100)
    want = R.cut_and_rebase(host_ds, ids)
    assert len(ids) > 4095 and 4 * len(want["senders"]) > 2 ** 20
    _no_build(monkeypatch)
    got = _graph_outputs(dev_ds.batch_of(ids))
    for k in R.ASSEMBLE_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k


def test_ids_outside_the_split_raise(dev_ds):
    g = len(dev_ds.all)
    for ids, split in (([g], None), ([-1], None), ([len(dev_ds.train_ids)], "train"), ([0], "test")):
        with pytest.raises(ValueError):
            dev_ds.batch_of(ids, split=split)
    tr = dev_ds.get_next_train_batch(5)
    te = dev_ds.get_random_test_batch(3)
    assert tr.n_node.shape == (5,) and te.n_node.shape == (3,) and tr.nodes.shape == (int(tr.n_node.sum()), 4)
    assert set(te.n_node.tolist()) <= {int(dev_ds.all.n_node[i]) for i in dev_ds.test_ids}
    # the ids come from the same numpy stream as GraphDataset.sample_ids; the features from a device generator of their own
    a, b = D.DeviceGraphDataset(dev_ds.all, 4, seed=3, device=DEV), D.DeviceGraphDataset(dev_ds.all, 4, gaussian_scale=2.0, seed=3, device=DEV)
    ga, gb = a.get_next_train_batch(6), b.get_next_train_batch(6)
    assert torch.equal(ga.n_node, gb.n_node) and torch.equal(ga.nodes * 2.0, gb.nodes)
    assert ga.n_node.tolist() == [int(a.all.n_node[i]) for i in np.random.default_rng(3).choice(a.train_ids, size=6, replace=True)]


# ---- gnf_complete_batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[], [1], R.COMPLETE_SIZES, R.COMPLETE_GRID, [361] * 5 + [3], [0, 3, 0, 0, 5, 0]],
                         ids=["empty", "single", "mixed", "grid361", "four_groups", "empty_graphs"])
def test_complete_batch_equals_transform_example_and_both_csrs(sizes, monkeypatch):
    n = int(np.sum(sizes, dtype=np.int64))
    x = torch.randn(n, 6, device=DEV)
    if len(sizes):
        parent = D.transform_example(x.cpu().numpy(), sizes, DEV)
    else:   # transform_example cannot concatenate zero graphs: the same empty batch, spelt out
        none = np.zeros(0, np.int32)
        parent = graph_from_arrays(none, none, none, none, x.cpu().numpy(), DEV)
    e = int(parent.senders.shape[0])
    pc, pt = build_csr_device(parent), build_csr_device(parent, by_sender=True)
    want = R.complete_closed_form(sizes)
    _no_build(monkeypatch)
    g = D.complete_batch(x, sizes, DEV)
    csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
    torch.cuda.synchronize()
    assert g.nodes.data_ptr() == x.data_ptr()                                   # a device tensor is used as it is
    for k in ("senders", "receivers", "n_node", "n_edge"):
        assert getattr(g, k).dtype == torch.int32 and torch.equal(getattr(g, k), getattr(parent, k).to(torch.int32)), k
    assert g.edges.shape == (e,) and g.globals.shape == (len(sizes),) and not g.edges.any()
    assert torch.equal(csr.rowptr, pc.rowptr) and torch.equal(csr_t.rowptr, pt.rowptr)
    assert torch.equal(csr.col[:e], pc.col[:e]) and torch.equal(csr_t.col[:e], pt.col[:e])
    assert csr.n_nodes == n and csr.n_edges == e
    if e:   # one array three times: both cache entries were seeded with the receivers tensor itself
        assert csr.col.data_ptr() == g.receivers.data_ptr() == csr_t.col.data_ptr()
    got = dict(node_offsets=node_offsets_of(g), n_edge=g.n_edge, rowptr=csr.rowptr, senders=g.senders, receivers=g.receivers)
    for k in R.COMPLETE_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_complete_batch_raw_leaves_guard_bands_untouched(shift):
    sizes = R.COMPLETE_SIZES
    want = R.complete_closed_form(sizes)
    b, n, e = len(sizes), int(want["node_offsets"][-1]), len(want["senders"])
    lib = _abi.lib()
    ws_bytes = lib.gnf_complete_batch_workspace_bytes(b)
    for nn, ee in ((n, e), (n - 3, e - 500), (n + 3, e + 500)):     # sizes that do not match n_node: wrong numbers, guards intact
        out = Guarded([b + 1, b, nn + 1, ee, ee], [16 + (shift + k) % 4 for k in range(5)])
        ws = Guarded([(ws_bytes + 3) // 4], [64])
        _abi.check(lib.gnf_complete_batch(_abi.ptr(_t(np.asarray(sizes, np.int32))), b, nn, ee, *out.ptrs(), ws.ptrs()[0], ws_bytes,
                                          _abi.stream_ptr(torch.device(DEV))), "gnf_complete_batch")
        torch.cuda.synchronize()
        out.check()
        ws.check()
        if nn == n:
            for k, v in zip(R.COMPLETE_KEYS, out.views):
                assert torch.equal(v.cpu(), torch.from_numpy(want[k])), k


# ---- consumers see the same batch ----------------------------------------------------------------------------------------------------
DATA_ATTN = dict(num_heads=1, kq_dim=64, v_dim=64, out_dim=64, concat=True, kq_dim_division=True, residual=False)


def test_the_flow_gives_the_same_bits_on_a_complete_batch_graph():
    """the data-driver tests' flow (tests/test_data_driver_gpu.py): D = 200, dm_attn 1 x 64 / 64 / C 64, relu MLP 96 x 3, batch
    norm, T = 2"""
    from gnf_amd.flow import log_prob_terms
    d, latent, k, t = 200, 96, 3, 2
    sizes = [9, 4, 16, 7, 12]
    p = O.make_attn_grevnet_params(65, d // 2, latent, k, t, final_scale=0.3, **DATA_ATTN)
    p["bn"] = O.make_bn_params(66, d // 2, t)
    hp = dict(D=d, latent=latent, K=k, T=t, agg="mean", combine="agg", epsilon=0.0, activation="relu", weight_sharing=False,
              attn=DATA_ATTN)
    x = (np.random.default_rng(64).standard_normal((int(np.sum(sizes)), d)) * 0.9 + 0.1).astype(np.float32)
    outs = []
    for make in (D.transform_example, D.complete_batch):
        net = make_product_grevnet(hp, p)
        graph = make(x, sizes, DEV)
        terms = log_prob_terms(net, graph)
        back = net(graph.replace(nodes=terms["z_graph"].nodes), inverse=False).nodes
        torch.cuda.synchronize()
        outs.append((terms["z_graph"].nodes, terms["log_prob_xs_per_node"], back))
    for a, b in zip(*outs):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    assert bool(torch.isfinite(outs[0][0]).all())


def test_the_encoder_trainer_gives_the_same_loss_and_gradient_bits():
    from gnf_amd import encoder
    from gnf_amd.train import EncoderTrainer
    ds = D.DeviceGraphDataset("graph_rnn_grid_small", 6, device=DEV)
    ids = [6, 0, 7, 2, 6, 9]
    n = int(ds.all.n_node[ids].sum())
    x = torch.as_tensor((np.random.default_rng(7).standard_normal((n, 6)) * 0.3).astype(np.float32)).to(DEV)
    host = graphs_tuple_from_edge_lists(ds.all.n_node, ds.all.n_edge, ds.all.senders, ds.all.receivers, ids, x.cpu().numpy(), DEV)
    enc = encoder.make_encoder(dict(node_dim=6, latent=16, K=2, activation="leaky_relu", num_timesteps=2, agg="mean", combine="agg",
                                    epsilon=2.0))
    tr = EncoderTrainer(enc)
    res = []
    for graph in (host, ds.batch_of(ids, nodes=x)):
        out = tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        res.append((torch.as_tensor(out["sum_loss"]).clone(), tr.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(res[0][1].any()) and bool(torch.isfinite(res[0][1]).all())


# ---- chunk readers on a device -----------------------------------------------------------------------------------------------------------
def test_chunk_readers_on_a_device_hand_out_views_of_one_tensor_per_chunk(tmp_path):
    rng = np.random.default_rng(5)
    for k in range(2):
        n_node = rng.integers(2, 9, size=7).astype(np.int32)
        D.write_embedding_chunk(os.path.join(str(tmp_path), f"chunk_{k}.pkl"), rng.standard_normal((int(n_node.sum()), 3)), n_node)
    for make in (lambda **kw: D.GrevnetDatasetFixed(str(tmp_path), 3, sort_files=True, **kw),
                 lambda **kw: D.GrevnetDatasetVariable(str(tmp_path), 20, sort_files=True, **kw)):
        host, dev = make(), make(device=DEV)
        storages, next_ptr, batches = {}, {}, 0
        while True:
            try:
                hz, hn = host.train_batch()
            except IndexError:
                break
            dz, dn = dev.train_batch()
            batches += 1
            assert dev.file_ind == host.file_ind and isinstance(dn, np.ndarray) and np.array_equal(dn, hn)
            assert isinstance(dz, torch.Tensor) and dz.device == torch.device(DEV) and dz.dtype == torch.float32
            assert torch.equal(dz.cpu(), torch.from_numpy(hz.astype(np.float32)))
            store = dz.untyped_storage().data_ptr()
            storages.setdefault(dev.file_ind, set()).add(store)
            # zero-copy: a chunk's first batch starts at its tensor's first row, every later one where the last one ended
            assert dz.data_ptr() == next_ptr.get(dev.file_ind, store)
            next_ptr[dev.file_ind] = dz.data_ptr() + dz.shape[0] * 3 * 4
        assert batches >= 4 and sorted(storages) == [0, 1] and all(len(v) == 1 for v in storages.values())
        with pytest.raises(IndexError):
            dev.train_batch()


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def _run(script, *flags):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *flags], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout


def test_run_gnn_with_device_batches(tmp_path):
    out = _run("run_gnn.py", "--dataset", "graph_rnn_grid_small", "--node_embedding_dim", "6", "--latent_dim", "16", "--num_layers", "2",
               "--num_processing_steps", "2", "--train_batch_size", "4", "--num_train_iters", "3", "--log_every_n_steps", "1",
               "--eval_every_n_steps", "2", "--save_path", str(tmp_path / "encoder.npz"), "--device_batches")
    assert "iteration num: 2" in out and "eval sum loss:" in out and "after 3 steps" in out


DATA_FLAGS = ("--make_chunks", "--attn_type", "avg_then_mlp", "--node_embedding_dim", "8", "--latent_dim", "16", "--num_layers", "2",
              "--num_coupling_layers", "2", "--train_batch_size", "4", "--num_train_iters", "2", "--log_every_n_steps", "1",
              "--sample_size", "2", "--clip_gradient_by_norm", "--device_batches")


@pytest.mark.parametrize("extra", [(), ("--variable_dataset", "--max_nodes", "60")], ids=["fixed", "variable"])
def test_train_grevnet_with_data_with_device_batches(extra):
    out = _run("train_grevnet_with_data.py", *DATA_FLAGS, *extra)
    assert "iteration     2" in out and "batch nodes" in out and "sampled graph 1" in out and "per-node NLL over the" in out
    if extra:   # fewer than 60 nodes per batch, whatever number of graphs that takes
        nodes = [int(line.rsplit("batch nodes", 1)[1]) for line in out.splitlines() if "batch nodes" in line]
        assert len(nodes) == 3 and all(0 < v < 60 for v in nodes)
