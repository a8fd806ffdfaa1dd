"""Edge-deletion noise without a device (include/gnf_perturb.h, datasets.perturb_batch / NoisyGraphDataset): header, exports and
binding in step; the hash's known answers and the threshold's ends; every rejection with its code and text before any launch;
the deletion rate of the definition; the numpy route of the package against the pure-Python restatement of
tests/perturb_ref.py; and the host NoisyGraphDataset."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import batches_ref as R
import perturb_ref as PR
from gnf_amd import _abi, datasets as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnf_perturb_edges_workspace_bytes", "gnf_perturb_edges")
GNF_EINVAL, GNF_ESHAPE, GNF_EWORKSPACE = -1, -2, -3
P = 1 << 20   # a made-up non-null pointer: every call below fails before any launch, nothing is dereferenced
SEEDS = (0, 1, 12345, 12346, 2 ** 63 + 5)
PROBS = (0.1, 0.3, 0.5, 0.9)


def test_symbols_are_exported_and_bound():
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_perturb.h"$', main, flags=re.M)
    assert re.search(r"^#define GNF_ABI_VERSION 10$", main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_perturb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.PERTURB_SYMBOLS)
    others = [getattr(_abi, name) for name in dir(_abi) if name.endswith("_SYMBOLS") and name != "PERTURB_SYMBOLS"]
    assert len(others) >= 13
    for other in others:
        assert not set(_abi.PERTURB_SYMBOLS) & set(other)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", own))) == sorted(_abi.EXPORTED_SYMBOLS)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    fields = re.search(r"typedef struct GnfPerturbSpec \{(.*?)\}", text, flags=re.S).group(1)
    names = [n.strip(" *") for n in re.findall(r"(?:double|uint64_t|const uint64_t\s*\*|int32_t)\s*([a-z_]+);", fields)]
    assert names == [f[0] for f in _abi.GnfPerturbSpec._fields_]
    assert re.search(r"GNF_PERTURB_LOOPS_KEEP = 0, GNF_PERTURB_LOOPS_DRAW = 1", text)
    assert (_abi.GNF_PERTURB_LOOPS_KEEP, _abi.GNF_PERTURB_LOOPS_DRAW) == (0, 1) == (D.PERTURB_LOOPS["keep"], D.PERTURB_LOOPS["draw"])
    flat = " ".join(raw.replace("\n * ", " ").split())
    for phrase in ("a symmetric graph stays symmetric", "different noise", "no owning-graph lookup", "never used as an index",
                   "wrong numbers, never an access outside the arrays", "0x9E3779B97F4A7C15", "0x94D049BB133111EB"):
        assert phrase.lower() in flat.lower(), phrase


def test_known_answers_of_the_draw():
    for seed, lo, hi, want in PR.KNOWN_ANSWERS:
        assert PR.draw(seed, lo, hi) == want
        assert int(D.perturb_draw(seed, lo, hi)[0]) == want
    lo = np.array([k[1] for k in PR.KNOWN_ANSWERS[1:3]])
    hi = np.array([k[2] for k in PR.KNOWN_ANSWERS[1:3]])
    assert D.perturb_draw(0, lo, hi).tolist() == [PR.draw(0, int(a), int(b)) for a, b in zip(lo, hi)]


def test_threshold_is_exact_at_the_ends():
    for p, want in ((0.0, 0), (1.0, 2 ** 32), (2.0 ** -32, 1), (1.0 - 2.0 ** -32, 2 ** 32 - 1), (0.3, int(0.3 * 2 ** 32))):
        assert PR.threshold(p) == want == D.perturb_threshold(p)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            D.perturb_threshold(bad)


def _call(edges=(P, P), n_edge=P, csr=(P, P, 10, 20, P, 4), csr_t=(P, P, 10, 20, P, 4), spec=(0.3, 12345, None, 0), outs=None,
          ws=P, ws_bytes=None, null_csr=False, null_csr_t=False, null_spec=False):
    lib = _abi.lib()
    c, ct, sp = _abi.GnfCsr(*csr), _abi.GnfCsr(*csr_t), _abi.GnfPerturbSpec(*spec)
    outs = [P] * 9 if outs is None else outs
    if ws_bytes is None:
        ws_bytes = max(lib.gnf_perturb_edges_workspace_bytes(max(csr[5], 0), max(csr[2], 0), max(min(csr[3], 2 ** 31 - 1), 0)), 8)
    rc = lib.gnf_perturb_edges(edges[0], edges[1], n_edge, None if null_csr else C.byref(c), None if null_csr_t else C.byref(ct),
                               None if null_spec else C.byref(sp), *outs, ws, ws_bytes, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def _none_at(k, count):
    return [None if i == k else P for i in range(count)]


def test_rejections_come_with_their_code_and_text():
    need = _abi.lib().gnf_perturb_edges_workspace_bytes(4, 10, 20)
    bad = [(dict(null_csr=True), GNF_EINVAL), (dict(null_csr_t=True), GNF_EINVAL), (dict(null_spec=True), GNF_EINVAL),
           (dict(edges=(None, P)), GNF_EINVAL), (dict(edges=(P, None)), GNF_EINVAL), (dict(n_edge=None), GNF_EINVAL),
           (dict(ws=None), GNF_EINVAL)]
    bad += [(dict(outs=_none_at(k, 9)), GNF_EINVAL) for k in range(9)]
    bad += [(dict(csr=(None, P, 10, 20, P, 4)), GNF_EINVAL), (dict(csr=(P, None, 10, 20, P, 4)), GNF_EINVAL),
            (dict(csr_t=(None, P, 10, 20, P, 4)), GNF_EINVAL), (dict(csr_t=(P, None, 10, 20, P, 4)), GNF_EINVAL),
            (dict(csr=(P, P, 10, 20, None, 4)), GNF_EINVAL), (dict(csr_t=(P, P, 10, 20, None, 4)), GNF_EINVAL),   # node_offsets
            (dict(spec=(0.3, 1, None, 2)), GNF_EINVAL), (dict(spec=(0.3, 1, None, -1)), GNF_EINVAL),
            (dict(spec=(-0.001, 1, None, 0)), GNF_EINVAL), (dict(spec=(1.001, 1, None, 0)), GNF_EINVAL),
            (dict(spec=(float("nan"), 1, None, 0)), GNF_EINVAL)]
    bad += [(dict(csr=(P, P, -1, 20, P, 4), csr_t=(P, P, -1, 20, P, 4)), GNF_ESHAPE),
            (dict(csr=(P, P, 10, -1, P, 4), csr_t=(P, P, 10, -1, P, 4)), GNF_ESHAPE),
            (dict(csr=(P, P, 10, 20, P, -1), csr_t=(P, P, 10, 20, P, -1)), GNF_ESHAPE),
            (dict(csr=(P, P, 2 ** 31, 20, P, 4), csr_t=(P, P, 2 ** 31, 20, P, 4)), GNF_ESHAPE),
            (dict(csr=(P, P, 10, 2 ** 31, P, 4), csr_t=(P, P, 10, 2 ** 31, P, 4)), GNF_ESHAPE),
            (dict(csr_t=(P, P, 10, 21, P, 4)), GNF_ESHAPE), (dict(csr_t=(P, P, 11, 20, P, 4)), GNF_ESHAPE),
            (dict(ws_bytes=need - 1), GNF_EWORKSPACE), (dict(ws_bytes=0), GNF_EWORKSPACE)]
    for kw, code in bad:
        rc, msg = _call(**kw)
        assert rc == code and msg.startswith("gnf_perturb_edges"), (kw, rc, msg)
    assert "workspace" in _call(ws_bytes=0)[1] and "null" in _call(n_edge=None)[1] and "node_offsets" in _call(
        csr=(P, P, 10, 20, None, 4))[1]
    assert "deletion_prob" in _call(spec=(2.0, 1, None, 0))[1] and "self_loops=2" in _call(spec=(0.3, 1, None, 2))[1]
    assert "n_nodes=-1" in _call(csr=(P, P, -1, 20, P, 4))[1]
    # the edge arrays may be NULL when E == 0: that call gets past every check (and is not made here)


def test_workspace_size_is_a_monotone_host_computation():
    f = _abi.lib().gnf_perturb_edges_workspace_bytes
    assert f(0, 0, 0) == 16                                   # base[3][1] + eb[1]
    assert f(9, 100, 4486) == 3 * 71 * 8 + 3 * 72 * 4 + 10 * 4
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (1, 2 ** 31, 1), (1, 1, 2 ** 31), (2 ** 31, 1, 1)):
        assert f(*bad) == 0
    assert f(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) > 0
    for lo, hi in ((0, 1), (63, 64), (64, 65), (1024, 1025), (4486, 10 ** 6)):
        assert f(4, 10, lo) <= f(4, 10, hi) and f(lo, 10, 64) <= f(hi, 10, 64)
    assert f(4, 10, 64) == f(4, 5000, 64)                     # the rows need no workspace


# ---- the definition's deletion rate -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def complete200_draws():
    pairs = [(a, b) for a in range(200) for b in range(a + 1, 200)]
    assert len(pairs) == 19900
    return {seed: np.array([PR.draw(seed, a, b) for a, b in pairs], np.int64) for seed in SEEDS}


def test_deletion_rate_is_binomial(complete200_draws):
    n = 19900
    lo = np.array([a for a in range(200) for b in range(a + 1, 200)])
    hi = np.array([b for a in range(200) for b in range(a + 1, 200)])
    worst = 0.0
    for seed in SEEDS:
        assert np.array_equal(D.perturb_draw(seed, lo, hi), complete200_draws[seed])     # the numpy restatement, pair for pair
        for p in PROBS:
            share = float((complete200_draws[seed] < PR.threshold(p)).mean())
            dev = abs(share - p) / math.sqrt(p * (1 - p) / n)
            worst = max(worst, dev)
            assert dev <= 5.0, (seed, p, share, dev)
    print(f"worst deviation {worst:.3f} binomial standard deviations")
    # two neighbouring seeds are independent streams: deleted under both at p = 0.3 is 0.09 of all pairs
    thr = PR.threshold(0.3)
    both = float(((complete200_draws[12345] < thr) & (complete200_draws[12346] < thr)).mean())
    print(f"deleted under both seeds: {both:.4f}")
    assert abs(both - 0.09) <= 5.0 * math.sqrt(0.09 * 0.91 / n), both


# ---- perturb_batch on CPU batches against the restatement -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_ds():
    return R.dataset()


def _cpu_graph(t):
    from gnf_amd.graphs import GraphsTuple
    n, e = int(t["node_offsets"][-1]), len(t["senders"])
    return GraphsTuple(nodes=torch.zeros(n, 2), edges=torch.zeros(e), receivers=torch.from_numpy(t["receivers"].copy()),
                       senders=torch.from_numpy(t["senders"].copy()), globals=torch.zeros(len(t["n_node"])),
                       n_node=torch.from_numpy(t["n_node"].copy()), n_edge=torch.from_numpy(t["n_edge"].copy()))


@pytest.mark.parametrize("loops", ["keep", "draw"])
@pytest.mark.parametrize("name", ["mixed", "reversed", "one"])
def test_perturb_batch_on_cpu_equals_the_restatement(host_ds, name, loops):
    ids = R.id_lists(host_ds)[name]
    t = PR.batch(host_ds, ids)
    n = int(t["node_offsets"][-1])
    want = PR.perturb(t["senders"], t["receivers"], n, t["n_edge"], 0.3, 12345, loops)
    got = D.perturb_arrays_host(t["senders"], t["receivers"], n, t["n_edge"], 0.3, 12345, loops)
    assert sorted(got) == sorted(PR.KEYS) == sorted(D.PERTURB_KEYS)
    for k in PR.KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    graph = _cpu_graph(t)
    noisy, removed = D.perturb_batch(graph, 0.3, 12345, self_loops=loops)
    assert noisy.nodes is graph.nodes and noisy.n_node is graph.n_node and noisy.globals is graph.globals
    assert noisy.edges.shape == (int(want["totals"][0]),) and not noisy.edges.any()
    for k, v in (("senders", noisy.senders), ("receivers", noisy.receivers), ("n_edge", noisy.n_edge), ("num_removed", removed)):
        assert v.dtype == torch.int32 and np.array_equal(v.numpy(), want[k]), k
    # deletion is symmetric: (s, r) survives iff (r, s) would
    kept = set(zip(want["senders"].tolist(), want["receivers"].tolist()))
    for s, r in zip(t["senders"].tolist(), t["receivers"].tolist()):
        if (r, s) in kept:
            assert (s, r) in kept
    loops_before = int((t["senders"] == t["receivers"]).sum())
    loops_after = int((want["senders"] == want["receivers"]).sum())
    assert (loops_after == loops_before) if loops == "keep" else (loops_after <= loops_before)
    assert int(want["n_edge"].sum()) == int(want["totals"][0]) == int(want["rowptr"][-1]) == int(want["rowptr_t"][-1])
    assert int(want["num_removed"].sum()) == int(want["totals"][1]) and int(want["totals"].sum()) == len(t["senders"])


def test_the_ends_of_the_probability_range(host_ds):
    t = PR.batch(host_ds, R.id_lists(host_ds)["mixed"])
    graph = _cpu_graph(t)
    n = int(t["node_offsets"][-1])
    for loops in ("keep", "draw"):
        same, removed = D.perturb_batch(graph, 0.0, 12345, self_loops=loops)            # p = 0: the input arrays
        assert torch.equal(same.senders, graph.senders) and torch.equal(same.receivers, graph.receivers)
        assert torch.equal(same.n_edge, graph.n_edge) and not removed.any()
        got = D.perturb_arrays_host(t["senders"], t["receivers"], n, t["n_edge"], 0.0, 12345, loops)
        for k in ("rowptr", "col", "rowptr_t", "col_t"):
            assert np.array_equal(got[k], t[k]), k
    none = D.perturb_arrays_host(t["senders"], t["receivers"], n, t["n_edge"], 1.0, 12345, "draw")   # p = 1, loops drawn: nothing left
    assert none["totals"].tolist() == [0, len(t["senders"])] and not none["rowptr"].any() and not none["rowptr_t"].any()
    assert len(none["senders"]) == 0 and np.array_equal(none["num_removed"], t["n_edge"])
    only_loops = D.perturb_arrays_host(t["senders"], t["receivers"], n, t["n_edge"], 1.0, 12345, "keep")
    assert np.array_equal(only_loops["senders"], only_loops["receivers"])
    assert len(only_loops["senders"]) == int((t["senders"] == t["receivers"]).sum())
    with pytest.raises(ValueError):
        D.perturb_batch(graph, 1.5, 0)
    with pytest.raises(KeyError):
        D.perturb_batch(graph, 0.5, 0, self_loops="maybe")


def test_the_cases_have_what_they_are_there_for(host_ds):
    ids = R.id_lists(host_ds)["mixed"]
    t = PR.batch(host_ds, ids)
    n, e = int(t["node_offsets"][-1]), len(t["senders"])
    assert e == 4486
    keep = PR.perturb(t["senders"], t["receivers"], n, t["n_edge"], 0.3, 12345, "keep")
    draw = PR.perturb(t["senders"], t["receivers"], n, t["n_edge"], 0.3, 12345, "draw")
    assert int(keep["totals"][1]) == 1350 and int(draw["totals"][1]) == 1368

    def emptied(res):     # rows that had in-edges and have none afterwards
        return int(((np.diff(t["rowptr"]) > 0) & (np.diff(res["rowptr"]) == 0)).sum())
    assert emptied(keep) == 6 and emptied(draw) == 7
    loops = int((t["senders"] == t["receivers"]).sum())
    assert loops == 83 and loops - int((draw["senders"] == draw["receivers"]).sum()) == 18
    assert {R.COMPLETE, R.EDGELESS, R.LOOP_ONLY} <= set(ids)
    assert host_ds.n_edge[R.COMPLETE] == 65 * 65 > 64 * 64          # one graph spans more than 64 ballot words
    assert host_ds.n_edge[R.EDGELESS] == 0 and host_ds.n_edge[R.LOOP_ONLY] == 1
    slot = ids.index(R.LOOP_ONLY)
    assert keep["n_edge"][slot] == 1                                # the loop-only graph keeps its loop in keep mode


# ---- NoisyGraphDataset on the host ---------------------------------------------------------------------------------------------
def test_noisy_graph_dataset_on_the_host():
    ds = D.NoisyGraphDataset("graph_rnn_grid_small", 3, deletion_prob=0.3, seed=7)
    plain = D.GraphDataset("graph_rnn_grid_small", 3, seed=7)
    assert isinstance(ds, D.GraphDataset) and ds.on_device is None
    out = ds.get_next_train_batch(5)
    assert type(out) is tuple and len(out) == 3
    true, noisy, removed = out
    ref = plain.get_next_train_batch(5)
    for k in ("nodes", "senders", "receivers", "n_node", "n_edge"):      # the true batch is GraphDataset's batch
        assert torch.equal(getattr(true, k), getattr(ref, k)), k
    pairs = lambda g: list(zip(g.senders.tolist(), g.receivers.tolist()))
    assert set(pairs(noisy)) < set(pairs(true)) and noisy.nodes is true.nodes
    assert torch.equal(removed, true.n_edge - noisy.n_edge) and int(removed.sum()) > 0
    want = D.perturb_batch(true, 0.3, 7)[0]                                # the first call's seed is `seed`
    assert torch.equal(noisy.senders, want.senders) and torch.equal(noisy.receivers, want.receivers)
    # successive calls use different masks: the second call's seed is seed + 1
    true2, noisy2, _ = ds.get_next_train_batch(5)
    assert torch.equal(noisy2.senders, D.perturb_batch(true2, 0.3, 8)[0].senders)
    assert not torch.equal(noisy2.senders, D.perturb_batch(true2, 0.3, 7)[0].senders)
    # test batches are clean
    for test in (ds.get_next_test_batch(4), ds.get_random_test_batch(4)):
        assert type(test) is type(true) and int(test.n_edge.sum()) == test.senders.shape[0]
        assert set(test.n_node.tolist()) <= {int(ds.all.n_node[i]) for i in ds.test_ids}
    doc = " ".join(D.NoisyGraphDataset.__doc__.split())
    assert "ACTUALLY DELETES" in doc and "RETURNS THE NOISY BATCH" in doc
    with pytest.raises(ValueError):
        D.NoisyGraphDataset("graph_rnn_grid_small", 3, deletion_prob=1.5)
