"""The synthetic datasets' device generator on the MI355X (include/gnf_synthetic.h): the topology integer for integer against
the numpy restatement AND against the parent route run on the device (the edge list through build_csr_device twice); the seeded
caches; the raw entry points with guard bands at every misalignment, with padded node rows and with sizes that do not match;
node features against the float64 restatement at the header's tolerances; determinism, seeds and the device seed word; the
call replayed from a hipGraph; then the consumers - the flow, the trainer and the example driver with --device_batches."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from gnf_amd import _abi, gnn, grevnet_synthetic_data as S
from gnf_amd.graphs import build_csr_device, csr_of, data_dicts_to_graphs_tuple, node_offsets_of
from helpers import graph_from_arrays
from test_batches_gpu import Guarded, _leave_the_process_wide_generators_as_found, _no_build   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL_F = -12345.5
TOPOLOGY_KEYS = ("node_offsets", "n_edge", "rowptr", "senders", "receivers", "col")
SIZES = ([1], [2], [3, 1, 4], [0, 5, 0], [6, 10, 20], [100, 100])
MOONS_SIZES = [1, 2, 3, 6, 100]
MOG3 = S.SyntheticSpec("mog", offset_sets=[S.OFFSETS_4, S.OFFSETS_6, S.OFFSETS_9])
MOG3_ROTATE = S.SyntheticSpec("mog", offset_sets=[S.OFFSETS_4, S.OFFSETS_6, S.OFFSETS_9], rotate=True)
MOG3_SETS = [0, 1, 2, 2, 0]


def _t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _raw_topology(sizes, n=None, e=None, shift=0):
    """gnf_synthetic_topology into guard-banded outputs, output k misaligned by (shift + k) % 4 words"""
    want = S.synthetic_topology_host(sizes)
    b = len(sizes)
    n = int(want["node_offsets"][-1]) if n is None else n
    e = len(want["senders"]) if e is None else e
    lib = _abi.lib()
    ws_bytes = lib.gnf_synthetic_topology_workspace_bytes(b)
    out = Guarded([b + 1, b, n + 1, e, e, e], [16 + (shift + k) % 4 for k in range(6)])
    ws = Guarded([(ws_bytes + 3) // 4], [64])
    n_dev = _t(np.asarray(sizes, np.int32))
    _abi.check(lib.gnf_synthetic_topology(_abi.ptr(n_dev), b, n, e, *out.ptrs(), ws.ptrs()[0], ws_bytes,
                                          _abi.stream_ptr(torch.device(DEV))), "gnf_synthetic_topology")
    torch.cuda.synchronize()
    out.check()
    ws.check()
    return dict(zip(TOPOLOGY_KEYS, out.views)), want


def _c_spec(spec, seed, seed_tensor=None):
    """(GnfSyntheticSpec, whatever it points to)"""
    c = _abi.GnfSyntheticSpec()
    c.seed, c.seed_dev = int(seed) & (2 ** 64 - 1), None if seed_tensor is None else seed_tensor.data_ptr()
    c.kind, c.rotate, c.noise = (_abi.GNF_SYN_MOONS if spec.kind == "moons" else _abi.GNF_SYN_MOG), int(spec.rotate), spec.noise
    table = None
    if spec.kind == "mog":
        stride = max(spec.sizes)
        host = np.zeros((len(spec.offset_sets), stride, 2), np.float32)
        for q, o in enumerate(spec.offset_sets):
            host[q, :len(o)] = o
            c.set_size[q] = len(o)
        table = _t(host)
        c.offsets, c.n_sets, c.set_stride = table.data_ptr(), len(spec.offset_sets), stride
    return c, table


def _raw_nodes(spec, sizes, set_id, seed, seed_tensor=None, ld=2, n=None, max_n=None, want_source=True):
    """gnf_synthetic_nodes into a sentinel-filled [rows, ld] buffer with guard rows around it; returns (nodes [N, 2] view, source)"""
    sizes = np.asarray(sizes, np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(offs[-1]) if n is None else n
    c, keep = _c_spec(spec, seed, seed_tensor)
    lead = 7
    buf = torch.full(((n + 2 * lead) * ld,), SENTINEL_F, dtype=torch.float32, device=DEV)
    rows = buf[lead * ld:(lead + n) * ld].view(n, ld)
    src = Guarded([n], [17])
    n_dev, off_dev = _t(sizes), _t(offs)                      # (held until the call has run)
    set_dev = None if set_id is None else _t(np.asarray(set_id, np.int32))
    _abi.check(_abi.lib().gnf_synthetic_nodes(C.byref(c), _abi.ptr(n_dev), _abi.ptr(set_dev), _abi.ptr(off_dev), len(sizes), n,
                                              int(max(sizes.max(), 1)) if max_n is None else max_n, C.c_void_p(rows.data_ptr()), ld,
                                              src.ptrs()[0] if want_source else None, _abi.stream_ptr(torch.device(DEV))),
               "gnf_synthetic_nodes")
    torch.cuda.synchronize()
    src.check()
    assert bool((buf[:lead * ld] == SENTINEL_F).all()) and bool((buf[(lead + n) * ld:] == SENTINEL_F).all()), "guard rows changed"
    assert bool((rows[:, 2:] == SENTINEL_F).all()), "padding columns changed"
    return rows[:, :2], src.views[0]


# ---- topology ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
def test_topology_equals_the_restatement_and_the_parent_route(sizes):
    got, want = _raw_topology(sizes)
    for k in TOPOLOGY_KEYS:
        assert got[k].dtype == torch.int32 and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    n, e = int(want["node_offsets"][-1]), len(want["senders"])
    # the parent route on the device: the downloaded edge list as a GraphsTuple of its own, gnf_build_csr by receiver and by sender
    parent = graph_from_arrays(np.asarray(sizes, np.int32), got["n_edge"].cpu().numpy(), got["senders"].cpu().numpy(),
                               got["receivers"].cpu().numpy(), np.zeros((n, 2), np.float32), DEV)
    pc, pt = build_csr_device(parent), build_csr_device(parent, by_sender=True)
    torch.cuda.synchronize()
    assert torch.equal(pc.rowptr, got["rowptr"]) and torch.equal(pt.rowptr, got["rowptr"])
    assert torch.equal(pc.col[:e], got["col"]) and torch.equal(pt.col[:e], got["receivers"])


@pytest.mark.parametrize("name,batch", [("mom_6_10_20", 7), ("moons_100", 2), ("mog_4_9", 5), ("mog_6", 3)])
def test_a_dataset_batch_answers_csr_of_without_a_build(name, batch, monkeypatch):
    ds = S.DeviceSyntheticDataset(name, DEV, seed=77)
    ds.get_next_batch(batch)
    _no_build(monkeypatch)
    g = ds.get_next_batch(batch)                                  # batch 1: seed 78
    csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
    offsets = node_offsets_of(g)
    torch.cuda.synchronize()
    n_node, set_id = ds.spec.choose(batch, 78)
    want = S.synthetic_batch_host(ds.spec, n_node, set_id, 78)
    n, e = len(want["source"]), len(want["senders"])
    got = dict(node_offsets=offsets, n_edge=g.n_edge, rowptr=csr.rowptr, senders=g.senders, receivers=g.receivers, col=csr.col[:e],
               n_node=g.n_node, source=ds.last_source)
    for k, v in got.items():
        assert v.dtype == torch.int32 and torch.equal(v.cpu(), torch.from_numpy(want[k])), k
    assert torch.equal(csr_t.rowptr, csr.rowptr) and csr_t.col.data_ptr() == g.receivers.data_ptr()
    assert (csr.n_nodes, csr.n_edges, csr_t.n_nodes, csr_t.n_edges) == (n, e, n, e)
    assert g.nodes.shape == (n, 2) and g.nodes.dtype == torch.float32 and g.nodes.device == torch.device(DEV)
    assert g.edges.shape == (e,) and not g.edges.any() and g.globals.shape == (batch,) and not g.globals.any()
    again = ds.get_next_batch(batch)
    assert (again.senders is g.senders) == ds.spec.fixed_size and not torch.equal(again.nodes[:4], g.nodes[:4])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_raw_topology_leaves_guard_bands_untouched_at_every_misalignment(shift):
    sizes = [6, 10, 0, 20, 1, 3]
    got, want = _raw_topology(sizes, shift=shift)
    for k in TOPOLOGY_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    n, e = int(want["node_offsets"][-1]), len(want["senders"])
    for nn, ee in ((n - 3, e - 50), (n + 3, e + 50), (n, 0)):      # sizes that do not match n_node: wrong numbers, guards intact
        _raw_topology(sizes, n=nn, e=ee, shift=shift)


# ---- node features -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [2, 5])
@pytest.mark.parametrize("noise", [0.05, 0.0, 1.0])
def test_moons_equal_the_restatement(noise, ld):
    spec = S.SyntheticSpec("moons", MOONS_SIZES, noise=noise)
    nodes, source = _raw_nodes(spec, MOONS_SIZES, None, 12345, ld=ld)
    want = S.synthetic_batch_host(spec, MOONS_SIZES, None, 12345)
    assert torch.equal(source.cpu(), torch.from_numpy(want["source"]))
    err = float(np.abs(nodes.cpu().numpy().astype(np.float64) - want["nodes"]).max())
    print(f"moons noise={noise} ld={ld}: max |device - float64| = {err:.3e}")
    assert err <= 3e-6 + 1e-5 * noise, err


@pytest.mark.parametrize("spec,atol", [(MOG3, 1e-5), (MOG3_ROTATE, 4e-5)], ids=["plain", "rotate"])
def test_mixtures_equal_the_restatement(spec, atol):
    sizes = [spec.sizes[q] for q in MOG3_SETS]
    nodes, source = _raw_nodes(spec, sizes, MOG3_SETS, 12345, ld=3)
    want = S.synthetic_batch_host(spec, sizes, MOG3_SETS, 12345)
    assert torch.equal(source.cpu(), torch.from_numpy(want["source"]))
    err = float(np.abs(nodes.cpu().numpy().astype(np.float64) - want["nodes"]).max())
    print(f"mog rotate={spec.rotate}: max |device - float64| = {err:.3e}")
    assert err <= atol, err
    # a node index beyond the set's size takes offset (0, 0): nine nodes on the four-point set
    nodes, source = _raw_nodes(MOG3, [9], [0], 5)
    want = S.synthetic_batch_host(MOG3, [9], [0], 5)
    assert torch.equal(source.cpu(), torch.from_numpy(want["source"]))
    assert float(np.abs(nodes.cpu().numpy().astype(np.float64) - want["nodes"]).max()) <= 1e-5


def test_sizes_that_do_not_match_stay_inside_the_arrays():
    spec = S.SyntheticSpec("moons", MOONS_SIZES)
    n = sum(MOONS_SIZES)
    for nn in (n - 3, n + 3):
        _raw_nodes(spec, MOONS_SIZES, None, 1, ld=5, n=nn)                     # the guards are checked inside
    nodes, _ = _raw_nodes(spec, MOONS_SIZES, None, 1, max_n=6)                 # counts are clamped to the caller's bound
    assert bool((nodes[:12] != SENTINEL_F).all()) and bool((nodes[18:] == SENTINEL_F).all())
    _raw_nodes(spec, [-4, 6, 2 ** 30], None, 1, n=6, max_n=1024)               # a negative count is 0; a huge one is clamped
    _raw_nodes(MOG3, [4, 6], [-7, 99], 1)                                       # set ids are clamped into the table
    nodes, source = _raw_nodes(spec, MOONS_SIZES, None, 1, want_source=False)  # source is optional
    assert bool((nodes != SENTINEL_F).all())


def test_two_calls_give_the_same_bits_and_seeds_differ():
    spec = S.SYNTHETIC_SPECS["mom_6_10_20"]
    word = torch.tensor([424242], dtype=torch.int64, device=DEV)
    a, src_a = _raw_nodes(spec, [6, 10, 20], None, 424242)
    b, src_b = _raw_nodes(spec, [6, 10, 20], None, 424242)
    c, src_c = _raw_nodes(spec, [6, 10, 20], None, 0, seed_tensor=word)        # the word wins over the value
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(src_a, src_b) and torch.equal(src_a, src_c)
    assert int(word[0]) == 424242                                              # the kernels never write the seed word
    other, _ = _raw_nodes(spec, [6, 10, 20], None, 424243)
    for lo, hi in ((0, 6), (6, 16), (16, 36)):                                 # another seed changes every graph
        assert not torch.equal(a[lo:hi], other[lo:hi])
    d, src_d = _raw_nodes(spec, [20, 10], None, 424242)                        # a graph depends on (seed, slot, size) only
    assert torch.equal(a[6:16], d[20:30]) and torch.equal(src_a[6:16], src_d[20:30])
    # the C definition of the draw, through the kernels: source is the argsort of the restatement's keys
    keys = S.synthetic_draw(424242, 2, np.arange(20, dtype=np.uint64), 0)
    assert src_a[16:].cpu().numpy().tolist() == np.argsort(keys, kind="stable").tolist()


def test_a_captured_call_replays_with_the_seed_of_the_moment():
    spec, sizes, s0 = S.SYNTHETIC_SPECS["mom_6_10_20"], np.asarray([6, 20, 10, 6], np.int32), 9000
    eager = [_raw_nodes(spec, sizes, None, s0 + k)[0].clone() for k in range(3)]
    n = int(sizes.sum())
    word = torch.tensor([s0], dtype=torch.int64, device=DEV)
    c, _keep = _c_spec(spec, 0, word)
    n_dev, off_dev = _t(sizes), _t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    nodes = torch.zeros(n, 2, device=DEV)
    source = torch.zeros(n, dtype=torch.int32, device=DEV)

    def launch():
        _abi.check(_abi.lib().gnf_synthetic_nodes(C.byref(c), _abi.ptr(n_dev), None, _abi.ptr(off_dev), len(sizes), n, 20,
                                                  _abi.ptr(nodes), 2, _abi.ptr(source), _abi.stream_ptr(torch.device(DEV))),
                   "gnf_synthetic_nodes")
        word.add_(1)
    launch()                                                    # once eagerly (this consumes seed s0 - put it back)
    word.fill_(s0)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        launch()
    for k in range(3):
        nodes.fill_(-1.0)
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(nodes, eager[k]), k
    assert int(word[0]) == s0 + 3


# ---- consumers ---------------------------------------------------------------------------------------------------------------------
def _host_copy_of(g):
    """the same arrays through the host route: download, one data dict per graph, data_dicts_to_graphs_tuple"""
    n_node = g.n_node.cpu().numpy()
    n_edge = g.n_edge.cpu().numpy()
    x, s, r = g.nodes.cpu().numpy(), g.senders.cpu().numpy(), g.receivers.cpu().numpy()
    no = np.concatenate([[0], np.cumsum(n_node)])
    eo = np.concatenate([[0], np.cumsum(n_edge)])
    dicts = [{"n_node": int(n_node[b]), "nodes": x[no[b]:no[b + 1]], "senders": s[eo[b]:eo[b + 1]] - no[b],
              "receivers": r[eo[b]:eo[b + 1]] - no[b]} for b in range(len(n_node))]
    return data_dicts_to_graphs_tuple(dicts, DEV)


def test_the_flow_and_the_trainer_give_the_same_bits_as_on_the_host_route():
    from gnf_amd.train import GRevNetTrainer
    dev_graph = S.DeviceSyntheticDataset("mom_6_10", DEV, seed=31).get_next_batch(3)
    host_graph = _host_copy_of(dev_graph)
    assert torch.equal(host_graph.senders, dev_graph.senders) and torch.equal(host_graph.nodes, dev_graph.nodes)
    gnn.set_random_seed(5)
    mlp = partial(gnn.make_mlp_model, 16, 1, 2, gnn.leaky_relu, 0.1, 0.1)
    net = gnn.GRevNet(partial(gnn.avg_then_mlp_gnn, mlp, 1.0), 2, 2)
    outs = []
    for graph in (host_graph, dev_graph):
        z_graph, logdet = net.f(graph)
        torch.cuda.synchronize()
        outs.append((z_graph.nodes.clone(), logdet.clone(), net.last_sums.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all()) and not torch.equal(outs[0][0], dev_graph.nodes)
    tr = GRevNetTrainer(net)
    res = []
    for graph in (host_graph, dev_graph):
        out = tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        res.append((torch.as_tensor(out["total_loss"]).clone(), tr.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(res[0][1].any()) and bool(torch.isfinite(res[0][1]).all()) and bool(torch.isfinite(res[0][0]))


def test_run_grevnet_with_device_batches():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_grevnet.py"), "--device_batches", "--dataset", "moons_6",
                          "--make_gnn_fn", "avg_then_mlp", "--gnn_latent_dim", "16", "--gnn_num_layers", "2",
                          "--num_coupling_layers", "2", "--train_batch_size", "4", "--num_train_iters", "3",
                          "--log_every_n_steps", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"^total_loss: (\S+)$", run.stdout, flags=re.M)]
    assert len(losses) >= 3 and all(np.isfinite(losses)), run.stdout[-2000:]
    assert "iteration num: 2" in run.stdout and "per-node NLL over the 4 graphs" in run.stdout
    assert re.search(r"^samples: .* finite True$", run.stdout, flags=re.M), run.stdout[-500:]
