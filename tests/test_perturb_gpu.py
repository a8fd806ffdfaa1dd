"""Edge-deletion noise on the device (include/gnf_perturb.h, datasets.perturb_batch / NoisyGraphDataset): every output integer for
integer against tests/perturb_ref.py AND against the host route run on the device (filtered list, build_csr_device twice); the
seeded caches; the raw entry point with guard bands at every 16-byte misalignment and at word / tile edges; inputs that do not
describe the batch; determinism, seeds and the device seed word; the capturable form replayed from a hipGraph; then the
consumers - the encoder's trainer, NoisyGraphDataset and the example driver with --denoising."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batches_ref as R
import perturb_ref as PR
from gnf_amd import _abi, datasets as D, graphs
from gnf_amd.graphs import build_csr_device, csr_desc, csr_of, graphs_tuple_from_edge_lists, node_offsets_of
from helpers import graph_from_arrays
# the guard-banded output buffers and the fixture that puts the process-wide generators back, as the batch-assembly tests have them
from test_batches_gpu import Guarded, _leave_the_process_wide_generators_as_found   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_KEYS = ("senders", "receivers", "col", "col_t")


@functools.lru_cache(maxsize=None)
def _host_ds():
    return R.dataset()


@functools.lru_cache(maxsize=None)
def _true(name):
    """the true batch of an id list of batches_ref (computed once, never changed)"""
    return PR.batch(_host_ds(), R.id_lists(_host_ds())[name])


@functools.lru_cache(maxsize=None)
def _want(name, p, seed, loops):
    t = _true(name)
    return PR.perturb(t["senders"], t["receivers"], int(t["node_offsets"][-1]), t["n_edge"], p, seed, loops)


@pytest.fixture(scope="module")
def dev_ds():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return D.DeviceGraphDataset(_host_ds(), 4, device=DEV)


def _no_build(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("gnf_build_csr ran: the CSR cache was not seeded")
    monkeypatch.setattr(graphs, "build_csr_device", refuse)


def _equal(got, want, k):
    assert got.dtype in (torch.int32, torch.int64) and torch.equal(got.cpu(), torch.from_numpy(np.asarray(want)).to(got.dtype)), k


# ---- perturb_batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loops", ["keep", "draw"])
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name", ["empty", "one", "mixed", "reversed", "drawn64"])
def test_perturb_batch_equals_the_reference_and_the_host_route(dev_ds, name, p, loops, monkeypatch):
    ids = R.id_lists(_host_ds())[name]
    t, want = _true(name), _want(name, p, 12345, loops)
    n, e2 = int(t["node_offsets"][-1]), int(want["totals"][0])
    # the host route on the device: the filtered list uploaded, gnf_build_csr twice
    parent = graph_from_arrays(t["n_node"], want["n_edge"], want["senders"], want["receivers"], np.zeros((n, 4), np.float32), DEV)
    pc, pt = build_csr_device(parent), build_csr_device(parent, by_sender=True)
    true = dev_ds.batch_of(ids, nodes=torch.zeros(n, 4, device=DEV))
    _no_build(monkeypatch)        # from here on every CSR is a cache hit: the true batch's and the noisy batch's
    noisy, removed = D.perturb_batch(true, p, 12345, self_loops=loops)
    csr, csr_t = csr_of(noisy), csr_of(noisy, by_sender=True)
    torch.cuda.synchronize()
    assert noisy.nodes is true.nodes and noisy.n_node is true.n_node and noisy.globals is true.globals
    assert noisy.edges.shape == (e2,) and noisy.edges.dtype == torch.float32 and not noisy.edges.any()
    assert noisy.senders.shape == (e2,) and noisy.receivers.shape == (e2,)
    assert e2 == 0 or noisy.senders.data_ptr() != true.senders.data_ptr()
    assert (csr.n_nodes, csr.n_edges, csr_t.n_nodes, csr_t.n_edges) == (n, e2, n, e2)
    assert node_offsets_of(noisy) is node_offsets_of(true)
    got = dict(senders=noisy.senders, receivers=noisy.receivers, rowptr=csr.rowptr, col=csr.col[:e2], rowptr_t=csr_t.rowptr,
               col_t=csr_t.col[:e2], n_edge=noisy.n_edge, num_removed=removed)
    for k, v in got.items():
        _equal(v, want[k], k)
    assert torch.equal(csr.rowptr, pc.rowptr) and torch.equal(csr_t.rowptr, pt.rowptr)
    assert torch.equal(csr.col[:e2], pc.col[:e2]) and torch.equal(csr_t.col[:e2], pt.col[:e2])
    if p == 0.0:
        assert e2 == len(t["senders"]) and torch.equal(noisy.senders, true.senders) and torch.equal(csr.col[:e2], csr_of(true).col[:e2])
    if p == 1.0 and loops == "draw":
        assert e2 == 0 and not csr.rowptr.any() and not csr_t.rowptr.any()


def test_a_batch_with_nodes_and_no_edge(dev_ds, monkeypatch):
    """E == 0 with N > 0: no ballot word at all, the scan and the row pointers still run"""
    ids = [R.EDGELESS, R.EDGELESS]
    true = dev_ds.batch_of(ids)
    _no_build(monkeypatch)
    noisy, removed = D.perturb_batch(true, 0.3, 12345)
    csr, csr_t = csr_of(noisy), csr_of(noisy, by_sender=True)
    assert noisy.senders.shape == (0,) and removed.tolist() == [0, 0] and noisy.n_edge.tolist() == [0, 0]
    assert csr.rowptr.shape == (9,) and not csr.rowptr.any() and not csr_t.rowptr.any() and csr.n_edges == 0
    g = _raw(true, csr_of(true), csr_of(true, by_sender=True), 0.3, 12345, "draw", shift=1)
    assert g["totals"].tolist() == [0, 0] and not g["rowptr"].any() and not g["rowptr_t"].any() and not g["num_removed"].any()


# ---- the raw entry point ---------------------------------------------------------------------------------------------------------
OUT_KEYS = ("senders", "receivers", "rowptr", "col", "rowptr_t", "col_t", "n_edge", "num_removed")


def _raw(g, csr, csr_t, p, seed, loops, shift=0, seed_dev=None, rowptr=None, rowptr_t=None, n_edge=None):
    """gnf_perturb_edges on the device batch g with guard bands around every output, the totals and the workspace; returns the
    outputs under the header's names (full capacity) - the bands are checked here"""
    b, n, e = int(g.n_node.shape[0]), int(g.nodes.shape[0]), int(g.senders.shape[0])
    lib = _abi.lib()
    out = Guarded([e, e, n + 1, e, n + 1, e, b, b], [16 + (shift + k) % 4 for k in range(8)])
    tot = Guarded([4], [16])                                  # int64 [2]
    ws_bytes = lib.gnf_perturb_edges_workspace_bytes(b, n, e)
    ws = Guarded([(ws_bytes + 3) // 4], [64])
    d, d_t = csr_desc(g, csr, node_offsets=True), csr_desc(g, csr_t, node_offsets=True)
    if rowptr is not None:
        d.rowptr, d_t.rowptr = rowptr.data_ptr(), rowptr_t.data_ptr()
    spec = _abi.GnfPerturbSpec(p, seed, 0 if seed_dev is None else seed_dev.data_ptr(), D.PERTURB_LOOPS[loops])
    ep = lambda x: _abi.ptr(x if e else None)
    _abi.check(lib.gnf_perturb_edges(ep(g.senders), ep(g.receivers), _abi.ptr(g.n_edge if n_edge is None else n_edge), C.byref(d),
                                     C.byref(d_t), C.byref(spec), *out.ptrs(), tot.ptrs()[0], ws.ptrs()[0], ws_bytes,
                                     _abi.stream_ptr(torch.device(DEV))), "gnf_perturb_edges")
    torch.cuda.synchronize()
    out.check(), tot.check(), ws.check()
    res = dict(zip(OUT_KEYS, out.views))
    res["totals"] = tot.views[0].view(torch.int64)
    return res


def _check_raw(got, want):
    e2 = int(want["totals"][0])
    assert got["totals"].tolist() == want["totals"].tolist()
    for k in OUT_KEYS:
        _equal(got[k][:e2] if k in EDGE_KEYS else got[k], want[k], k)


@functools.lru_cache(maxsize=None)
def _cut(e):
    """one 65-node graph holding the first e entries of the complete graph's sender-major edge list: (true arrays, reference)"""
    a = np.arange(65, dtype=np.int32)
    s, r = np.repeat(a, 65)[:e].copy(), np.tile(a, 65)[:e].copy()
    return (np.array([65], np.int32), np.array([e], np.int32), s, r), PR.perturb(s, r, 65, [e], 0.3, 12345, "draw")


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["mixed", "all_stay", "none_stay", "cut64", "cut65", "cut1024", "cut1025"])
def test_raw_entry_point_leaves_guard_bands_untouched_at_every_misalignment(dev_ds, case, shift):
    if case.startswith("cut"):
        (nn, ne, s, r), want = _cut(int(case[3:]))
        assert len(s) == int(case[3:]) and 0 < int(want["totals"][0]) < len(s)
        g = graph_from_arrays(nn, ne, s, r, np.zeros((65, 1), np.float32), DEV)
        csr, csr_t, p, loops = build_csr_device(g), build_csr_device(g, by_sender=True), 0.3, "draw"
    else:
        p, loops = {"mixed": (0.3, "keep"), "all_stay": (0.0, "draw"), "none_stay": (1.0, "draw")}[case]
        want = _want("mixed", p, 12345, loops)
        g = dev_ds.batch_of(R.id_lists(_host_ds())["mixed"])
        csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
        e = int(g.senders.shape[0])
        assert int(want["totals"][0]) == {"mixed": e - 1350, "all_stay": e, "none_stay": 0}[case]
    _check_raw(_raw(g, csr, csr_t, p, 12345, loops, shift), want)


def test_arrays_that_do_not_describe_the_batch_stay_inside_the_arrays(dev_ds):
    g = dev_ds.batch_of(R.id_lists(_host_ds())["mixed"])
    csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
    n, e = int(g.nodes.shape[0]), int(g.senders.shape[0])
    rng = np.random.default_rng(3)
    wild = lambda: torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31 - 1, size=n + 1).astype(np.int32)).to(DEV)
    # row pointers above E, below 0 and out of order; an n_edge that sums past E, with negative entries: some result, no band touched
    past = csr.rowptr.clone() + e
    _raw(g, csr, csr_t, 0.3, 12345, "keep", rowptr=past, rowptr_t=past.flip(0).contiguous())
    _raw(g, csr, csr_t, 0.3, 12345, "draw", rowptr=wild(), rowptr_t=wild())
    big = torch.full_like(g.n_edge, 2 ** 31 - 1)
    big[1] = -7
    got = _raw(g, csr, csr_t, 0.3, 12345, "keep", n_edge=big)
    assert int(got["n_edge"].min()) >= 0 and int(got["num_removed"].min()) >= 0 and int(got["n_edge"].sum()) <= e
    _raw(g, csr, csr_t, 0.3, 12345, "keep", n_edge=g.n_edge * 3)


def test_two_calls_give_the_same_bits_and_seeds_differ(dev_ds):
    g = dev_ds.batch_of(R.id_lists(_host_ds())["mixed"])
    csr, csr_t = csr_of(g), csr_of(g, by_sender=True)
    a, b = _raw(g, csr, csr_t, 0.3, 12345, "keep"), _raw(g, csr, csr_t, 0.3, 12345, "keep", shift=2)
    other = _raw(g, csr, csr_t, 0.3, 12346, "keep")
    e2 = int(a["totals"][0])
    for k in OUT_KEYS:
        assert torch.equal(a[k][:e2] if k in EDGE_KEYS else a[k], b[k][:e2] if k in EDGE_KEYS else b[k]), k
    assert torch.equal(a["totals"], b["totals"])
    _check_raw(other, _want("mixed", 0.3, 12346, "keep"))
    assert not torch.equal(a["num_removed"], other["num_removed"]) and not torch.equal(a["rowptr"], other["rowptr"])
    # the seed word on the device is the host seed: 12345 there equals seed = 12345, whatever the host value says
    word = torch.tensor([12345], dtype=torch.int64, device=DEV)
    _check_raw(_raw(g, csr, csr_t, 0.3, 777, "keep", seed_dev=word), _want("mixed", 0.3, 12345, "keep"))
    word.fill_(2 ** 63 + 5 - 2 ** 64)                    # the bits of 2^63 + 5
    _check_raw(_raw(g, csr, csr_t, 0.3, 777, "keep", seed_dev=word), _want("mixed", 0.3, 2 ** 63 + 5, "keep"))


def test_the_capturable_form_replays_with_the_seed_of_the_moment(dev_ds):
    true = dev_ds.batch_of(R.id_lists(_host_ds())["mixed"])
    csr_of(true), csr_of(true, by_sender=True), node_offsets_of(true)
    word = torch.tensor([12345], dtype=torch.int64, device=DEV)
    eager = {}
    for seed in (12345, 12346):
        noisy, removed = D.perturb_batch(true, 0.3, seed)
        eager[seed] = (noisy, removed, csr_of(noisy), csr_of(noisy, by_sender=True))
    D.perturb_batch(true, 0.3, 0, seed_tensor=word, exact=False)      # the form that is captured, once eagerly
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        noisy_c, removed_c, info = D.perturb_batch(true, 0.3, 0, seed_tensor=word, exact=False)
    e = int(true.senders.shape[0])
    assert noisy_c.senders.shape == (e,) and noisy_c.edges.shape == (e,) and info["total_edges"].dtype == torch.int64
    for seed in (12345, 12346, 12345):
        word.fill_(seed)
        for v in (noisy_c.senders, noisy_c.receivers, info["col"], info["col_t"], info["rowptr"], info["rowptr_t"], removed_c):
            v.fill_(-1)
        cg.replay()
        torch.cuda.synchronize()
        noisy, removed, csr, csr_t = eager[seed]
        e2 = int(info["total_edges"])
        assert e2 == int(noisy.senders.shape[0]) == int(_want("mixed", 0.3, seed, "keep")["totals"][0])
        assert torch.equal(noisy_c.senders[:e2], noisy.senders) and torch.equal(noisy_c.receivers[:e2], noisy.receivers)
        assert torch.equal(info["col"][:e2], csr.col[:e2]) and torch.equal(info["col_t"][:e2], csr_t.col[:e2])
        assert torch.equal(info["rowptr"], csr.rowptr) and torch.equal(info["rowptr_t"], csr_t.rowptr)
        assert torch.equal(noisy_c.n_edge, noisy.n_edge) and torch.equal(removed_c, removed)


# ---- consumers --------------------------------------------------------------------------------------------------------------------
def test_the_encoder_trainer_gives_the_same_bits_as_on_a_host_built_noisy_batch():
    from gnf_amd import encoder
    from gnf_amd.train import EncoderTrainer
    ds = D.DeviceGraphDataset("graph_rnn_grid_small", 6, device=DEV)
    ids = [6, 0, 7, 2, 6, 9]
    t = PR.batch(ds.all, ids)
    n = int(t["node_offsets"][-1])
    want = PR.perturb(t["senders"], t["receivers"], n, t["n_edge"], 0.3, 12345, "keep")
    assert 0 < int(want["totals"][1]) < len(t["senders"])
    x = torch.as_tensor((np.random.default_rng(7).standard_normal((n, 6)) * 0.3).astype(np.float32)).to(DEV)
    host_true = graphs_tuple_from_edge_lists(ds.all.n_node, ds.all.n_edge, ds.all.senders, ds.all.receivers, ids, x.cpu().numpy(), DEV)
    host_noisy = graph_from_arrays(t["n_node"], want["n_edge"], want["senders"], want["receivers"], x.cpu().numpy(), DEV)
    true = ds.batch_of(ids, nodes=x)
    noisy, _ = D.perturb_batch(true, 0.3, 12345)
    enc = encoder.make_encoder(dict(node_dim=6, latent=16, K=2, activation="leaky_relu", num_timesteps=2, agg="mean", combine="agg",
                                    epsilon=2.0))
    tr = EncoderTrainer(enc)
    res = []
    for graph, truth in ((host_noisy, host_true), (noisy, true)):
        out = tr.loss_and_grads(graph, truth)
        torch.cuda.synchronize()
        keep = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
        keep["gnn_output.nodes"] = out["gnn_output"].nodes.clone()
        res.append((keep, tr.grad.clone(), tr.named_gradients()))
    (a, ga, na), (b, gb, nb) = res
    assert {"sum_loss", "mean_loss", "false_positive_pairs", "false_negative_pairs"} <= set(a) and sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ga, gb) and bool(ga.any()) and bool(torch.isfinite(ga).all())

    def leaves(x):
        if isinstance(x, dict):
            return [v for k in sorted(x) for v in leaves(x[k])]
        if isinstance(x, (list, tuple)):
            return [v for y in x for v in leaves(y)]
        return [np.asarray(x)]
    la, lb = leaves(na), leaves(nb)
    assert len(la) == len(lb) > 0 and all(np.array_equal(u, v) for u, v in zip(la, lb))
    # and the noise matters: the clean batch gives another loss
    clean = tr.loss_and_grads(true, true)
    assert not torch.equal(clean["sum_loss"], a["sum_loss"])


def test_noisy_graph_dataset_on_the_device_is_the_route_run_by_hand(monkeypatch):
    ds = D.NoisyGraphDataset("graph_rnn_grid_small", 5, deletion_prob=0.3, seed=11, device=DEV)
    hand = D.DeviceGraphDataset("graph_rnn_grid_small", 5, seed=11, device=DEV)
    assert isinstance(ds, D.GraphDataset) and isinstance(ds.on_device, D.DeviceGraphDataset)
    _no_build(monkeypatch)
    for call in range(2):
        true, noisy, removed = ds.get_next_train_batch(6)
        want_true = hand.get_next_train_batch(6)
        want_noisy, want_removed = D.perturb_batch(want_true, 0.3, 11 + call)
        for k in ("nodes", "senders", "receivers", "n_node", "n_edge"):
            assert torch.equal(getattr(true, k), getattr(want_true, k)), k
            assert torch.equal(getattr(noisy, k), getattr(want_noisy, k)), k
        assert torch.equal(removed, want_removed) and torch.equal(removed, true.n_edge - noisy.n_edge) and int(removed.sum()) > 0
        assert torch.equal(csr_of(noisy).rowptr, csr_of(want_noisy).rowptr)
        assert torch.equal(csr_of(noisy, by_sender=True).col, csr_of(want_noisy, by_sender=True).col)
    test = ds.get_random_test_batch(3)
    assert type(test) is type(true) and test.n_node.shape == (3,) and int(test.n_edge.sum()) == test.senders.shape[0]


def _run(script, *flags):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *flags], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout


@pytest.mark.parametrize("extra", [("--device_batches",), ()], ids=["device_batches", "host_batches"])
def test_run_gnn_denoising(tmp_path, extra):
    out = _run("run_gnn.py", "--dataset", "graph_rnn_community_small", "--node_embedding_dim", "6", "--latent_dim", "16",
               "--num_layers", "2", "--num_processing_steps", "2", "--train_batch_size", "4", "--num_train_iters", "3",
               "--log_every_n_steps", "1", "--eval_every_n_steps", "2", "--save_path", str(tmp_path / "encoder.npz"),
               "--denoising", "--deletion_prob", "0.3", *extra)
    assert "iteration num: 2" in out and "eval sum loss:" in out and "after 3 steps" in out
    lines = out.splitlines()
    heads = [i for i, line in enumerate(lines) if line == "NUM_NODES:NUM_REMOVED:NUM_INCORRECT"]
    assert len(heads) == 3                                                # one per training log; the evaluation keeps two columns
    assert sum(line == "NUM_NODES:NUM_INCORRECT" for line in lines) == 2
    for i in heads:
        cells = [c.split(":") for c in lines[i + 1].split(", ")]
        assert len(cells) == 4 and all(len(c) == 3 for c in cells)
        assert all(int(c[0]) > 0 and int(c[1]) >= 0 for c in cells) and sum(int(c[1]) for c in cells) > 0
