"""The synthetic datasets' device generator without a device (include/gnf_synthetic.h, grevnet_synthetic_data.
DeviceSyntheticDataset): header, exports and binding in step; the draw's known answers; the restatement's template against the
point set the sklearn test pins; its topology against the host route and a stable sort; the distributions at fixed seeds; every
rejection with its code and text before any launch; and the dataset class on the CPU."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import synthetic_ref as SR
from gnf_amd import _abi, grevnet_synthetic_data as S
from gnf_amd.graphs import build_csr_host, data_dicts_to_graphs_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnf_synthetic_topology_workspace_bytes", "gnf_synthetic_topology", "gnf_synthetic_nodes")
INLINE = ("gnf_syn_mix64", "gnf_syn_draw")
GNF_EINVAL, GNF_ESHAPE, GNF_EWORKSPACE = -1, -2, -3
P = 1 << 20   # a made-up non-null pointer: every call below fails before any launch, nothing is dereferenced
SIZES = ([1], [2], [3, 1, 4], [0, 5, 0], [6, 10, 20])


def test_symbols_are_exported_and_bound():
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_synthetic.h"$', main, flags=re.M)
    assert re.search(r"^#define GNF_ABI_VERSION 10$", main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_synthetic.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)) - set(INLINE))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.SYNTHETIC_SYMBOLS)
    for name in dir(_abi):
        if name.endswith("_SYMBOLS") and name != "SYNTHETIC_SYMBOLS":
            assert not set(_abi.SYNTHETIC_SYMBOLS) & set(getattr(_abi, name))
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    fields = re.search(r"typedef struct GnfSyntheticSpec \{(.*?)\}", text, flags=re.S).group(1)
    names = re.findall(r"([a-z_]+)(?:\[GNF_SYN_MAX_SETS\])?;", fields)
    assert names == [f[0] for f in _abi.GnfSyntheticSpec._fields_]
    assert re.search(r"GNF_SYN_MOONS = 0, GNF_SYN_MOG = 1", text) and (_abi.GNF_SYN_MOONS, _abi.GNF_SYN_MOG) == (0, 1)
    assert int(re.search(r"#define GNF_SYN_MAX_NODES (\d+)", text).group(1)) == _abi.GNF_SYN_MAX_NODES
    assert int(re.search(r"#define GNF_SYN_MAX_SETS (\d+)", text).group(1)) == _abi.GNF_SYN_MAX_SETS
    flat = " ".join(raw.replace("\n * ", " ").split())
    for phrase in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                   "wrong counts give wrong numbers, never an access outside the arrays", "THE ARRAY IDENTITY",
                   "grevnet_synthetic_data.py:17-21"):
        assert phrase.lower() in flat.lower(), phrase


def test_known_answers_of_the_draw():
    for seed, graph, index, stream, want in SR.KNOWN_ANSWERS:
        assert SR.draw(seed, graph, index, stream) == want
        assert int(S.synthetic_draw(seed, graph, index, stream)[0]) == want
    seeds, graphs = (0, 1, 12345, 2 ** 63 + 5, 2 ** 64 - 1), (0, 1, 31, 2 ** 20)
    indices, streams = (0, 1, 99, 1023, 2 ** 32 - 1), (0, 1, 2, 3, 4)
    for seed, graph in itertools.product(seeds, graphs):
        got = S.synthetic_draw(seed, graph, np.asarray(indices, np.uint64)[:, None], np.asarray(streams, np.uint64)[None, :])
        assert got.dtype == np.uint32
        assert got.tolist() == [[SR.draw(seed, graph, i, s) for s in streams] for i in indices]
    # the choice is the draw scaled: always inside [0, n_choices)
    for n in (1, 2, 3, 7):
        c = S.synthetic_choice(12345, 500, n)
        assert c.min() >= 0 and c.max() < n
        assert c.tolist() == [(SR.draw(12345, b, 0, 4) * n) >> 32 for b in range(500)]


def test_the_template_is_the_point_set_of_make_moons():
    spec = S.SyntheticSpec("moons", [1], noise=0.0)
    sizes = [1, 2, 3, 6, 10, 100]
    h = S.synthetic_batch_host(spec, sizes, None, 12345)
    for b, n in enumerate(sizes):
        lo, hi = h["node_offsets"][b], h["node_offsets"][b + 1]
        src = h["source"][lo:hi]
        assert sorted(src.tolist()) == list(range(n))
        assert np.abs(h["nodes"][lo:hi] - S._moons_template(n)[src]).max() <= 1e-15


def _host_route(sizes):
    dicts = []
    for n in sizes:
        # (the host function has no empty graph: its edge list is empty)
        s, r = S.fully_connected_edge_list(n) if n else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        dicts.append({"n_node": n, "senders": s, "receivers": r, "nodes": np.zeros((n, 2), np.float32)})
    return data_dicts_to_graphs_tuple(dicts)


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
def test_topology_of_the_restatement_is_the_host_route(sizes):
    t = S.synthetic_topology_host(sizes)
    g = _host_route(sizes)
    n = int(sum(sizes))
    for name in ("senders", "receivers", "n_edge"):
        assert t[name].dtype == np.int32 and np.array_equal(t[name], getattr(g, name).numpy()), name
    assert t["node_offsets"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rowptr, col = build_csr_host(t["senders"], t["receivers"], n)            # stable sort by receiver
    assert np.array_equal(t["rowptr"], rowptr) and np.array_equal(t["col"], col)
    rowptr_t, col_t = build_csr_host(t["receivers"], t["senders"], n)        # ... and by sender
    assert np.array_equal(t["rowptr"], rowptr_t) and np.array_equal(t["receivers"], col_t)
    assert np.array_equal(S.synthetic_topology_host([-3] + list(sizes))["senders"], t["senders"])   # a negative count is 0


def test_shuffle_is_uniform_over_permutations():
    h = S.synthetic_batch_host(S.SyntheticSpec("moons", [4], noise=0.0), [4] * 2400, None, 12345)
    index = {p: k for k, p in enumerate(itertools.permutations(range(4)))}
    counts = np.bincount([index[tuple(row)] for row in h["source"].reshape(2400, 4).tolist()], minlength=24)
    chi2 = float(((counts - 100.0) ** 2 / 100.0).sum())
    assert chi2 < 49.7, chi2   # the 99.9th percentile at 23 degrees of freedom


def test_noise_is_standard_normal():
    h = S.synthetic_batch_host(S.SyntheticSpec("moons", [100], noise=1.0), [100] * 64, None, 12345)
    res = h["nodes"] - S._moons_template(100)[h["source"]]      # every graph has the same template
    assert res.size == 12800
    assert abs(res.mean()) <= 5.0 / math.sqrt(12800), res.mean()
    assert abs(res.var() - 1.0) <= 5.0 * math.sqrt(2.0 / 12800), res.var()


def test_choices_are_uniform():
    n_node, set_id = S.SYNTHETIC_SPECS["mom_6_10_20"].choose(3000, 12345)
    assert not set_id.any()
    sd = math.sqrt(3000 * (1 / 3) * (2 / 3))
    for size in (6, 10, 20):
        assert abs(int((n_node == size).sum()) - 1000) <= 5 * sd, size
    n_node, set_id = S.SYNTHETIC_SPECS["mog_4_9"].choose(64, 7)
    assert set(set_id.tolist()) == {0, 1} and np.array_equal(n_node, np.where(set_id == 0, 4, 9))


def _topology(n_node=P, b=4, n=10, e=30, outs=None, ws=P, ws_bytes=None):
    lib = _abi.lib()
    outs = [P] * 6 if outs is None else outs
    if ws_bytes is None:
        ws_bytes = max(lib.gnf_synthetic_topology_workspace_bytes(max(b, 0)), 8)
    rc = lib.gnf_synthetic_topology(n_node, b, n, e, *outs, ws, ws_bytes, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def _spec(kind=0, noise=0.05, rotate=0, offsets=None, n_sets=0, stride=0, sizes=()):
    sp = _abi.GnfSyntheticSpec()
    sp.seed, sp.seed_dev, sp.kind, sp.rotate, sp.noise = 1, None, kind, rotate, noise
    sp.offsets, sp.n_sets, sp.set_stride = offsets, n_sets, stride
    for q, s in enumerate(sizes):
        sp.set_size[q] = s
    return sp


def _nodes(spec=None, null_spec=False, n_node=P, offsets=P, b=4, n=10, max_n=8, nodes=P, ld=2):
    lib = _abi.lib()
    spec = _spec() if spec is None else spec
    rc = lib.gnf_synthetic_nodes(None if null_spec else C.byref(spec), n_node, None, offsets, b, n, max_n, nodes, ld, None, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def test_rejections_come_with_their_code_and_text():
    need = _abi.lib().gnf_synthetic_topology_workspace_bytes(4)
    bad = [(dict(n_node=None), GNF_EINVAL), (dict(ws=None), GNF_EINVAL)]
    bad += [(dict(outs=[None if i == k else P for i in range(6)]), GNF_EINVAL) for k in range(6)]
    bad += [(dict(b=-1), GNF_ESHAPE), (dict(n=-1), GNF_ESHAPE), (dict(e=-1), GNF_ESHAPE), (dict(b=(1 << 20) + 1), GNF_ESHAPE),
            (dict(n=2 ** 31), GNF_ESHAPE), (dict(e=2 ** 31), GNF_ESHAPE),
            (dict(ws_bytes=need - 1), GNF_EWORKSPACE), (dict(ws_bytes=0), GNF_EWORKSPACE)]
    for kw, code in bad:
        rc, msg = _topology(**kw)
        assert rc == code and msg.startswith("gnf_synthetic_topology"), (kw, rc, msg)
    assert "workspace" in _topology(ws_bytes=0)[1] and "null" in _topology(n_node=None)[1] and "n_nodes=-1" in _topology(n=-1)[1]
    mog = dict(kind=1, offsets=P, n_sets=2, stride=9, sizes=(4, 9))
    bad = [(dict(null_spec=True), GNF_EINVAL), (dict(n_node=None), GNF_EINVAL), (dict(offsets=None), GNF_EINVAL),
           (dict(nodes=None), GNF_EINVAL), (dict(spec=_spec(kind=2)), GNF_EINVAL), (dict(spec=_spec(kind=-1)), GNF_EINVAL),
           (dict(spec=_spec(noise=-1e-9)), GNF_EINVAL), (dict(spec=_spec(noise=float("nan"))), GNF_EINVAL),
           (dict(spec=_spec(**{**mog, "offsets": None})), GNF_EINVAL), (dict(spec=_spec(**{**mog, "n_sets": 0})), GNF_EINVAL),
           (dict(spec=_spec(**{**mog, "n_sets": 9})), GNF_EINVAL), (dict(spec=_spec(**{**mog, "sizes": (4, 10)})), GNF_EINVAL),
           (dict(spec=_spec(**{**mog, "sizes": (-1, 9)})), GNF_EINVAL)]
    bad += [(dict(b=-1), GNF_ESHAPE), (dict(n=-1), GNF_ESHAPE), (dict(b=(1 << 20) + 1), GNF_ESHAPE), (dict(n=2 ** 31), GNF_ESHAPE),
            (dict(ld=1), GNF_ESHAPE), (dict(ld=-2), GNF_ESHAPE), (dict(max_n=0), GNF_ESHAPE),
            (dict(max_n=_abi.GNF_SYN_MAX_NODES + 1), GNF_ESHAPE)]
    for kw, code in bad:
        rc, msg = _nodes(**kw)
        assert rc == code and msg.startswith("gnf_synthetic_nodes"), (kw, rc, msg)
    assert "noise" in _nodes(spec=_spec(noise=-1.0))[1] and "kind=2" in _nodes(spec=_spec(kind=2))[1]
    assert "ld=1" in _nodes(ld=1)[1] and "max_nodes_per_graph=0" in _nodes(max_n=0)[1]
    assert "n_sets=9" in _nodes(spec=_spec(**{**mog, "n_sets": 9}))[1]
    # an empty batch gets past every check and launches nothing: GNF_OK with no pointer but the spec
    assert _nodes(n_node=None, offsets=None, nodes=None, b=0, n=0)[0] == 0
    assert _nodes(n_node=None, offsets=None, nodes=None, b=3, n=0)[0] == 0


def test_workspace_size_is_a_monotone_host_computation():
    f = _abi.lib().gnf_synthetic_topology_workspace_bytes
    sizes = [f(b) for b in (0, 1, 2, 31, 32, 33, 4095, 4096, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] >= 4 and all(s % 8 == 0 for s in sizes)
    assert f(32) >= 33 * 4
    assert f(-1) == 0 and f((1 << 20) + 1) == 0


def _same_graph(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in a._fields)


def test_the_dataset_on_the_cpu():
    for name in S.DATASETS_MAP:
        assert name in S.SYNTHETIC_SPECS
    ds = S.DeviceSyntheticDataset("mom_6_10_20", "cpu", seed=100)
    g0, src0 = ds.get_next_batch(5), ds.last_source
    g1 = ds.get_next_batch(5)
    for t, g in ((0, g0), (1, g1)):      # batch t uses seed + t
        n_node, set_id = ds.spec.choose(5, 100 + t)
        h = S.synthetic_batch_host(ds.spec, n_node, set_id, 100 + t)
        assert np.array_equal(g.nodes.numpy(), h["nodes"].astype(np.float32)) and g.nodes.dtype == torch.float32
        for f in ("senders", "receivers", "n_node", "n_edge"):
            assert np.array_equal(getattr(g, f).numpy(), h[f]) and getattr(g, f).dtype == torch.int32
        assert g.edges.shape == (len(h["senders"]),) and not g.edges.any() and g.globals.shape == (5,) and not g.globals.any()
    assert _same_graph(S.DeviceSyntheticDataset("mom_6_10_20", "cpu", seed=101).get_next_batch(5), g1)
    assert src0.dtype == torch.int32 and src0.shape[0] == g0.nodes.shape[0]
    # fixed-size datasets hand out the same index arrays every time
    for name in ("moons_6", "mog_4_rotate"):
        ds = S.DeviceSyntheticDataset(name, "cpu")
        a, b = ds.get_next_batch(3), ds.get_next_batch(3)
        assert a.senders is b.senders and a.receivers is b.receivers and a.n_node is b.n_node and a.n_edge is b.n_edge
        assert not torch.equal(a.nodes, b.nodes)
        assert ds.get_next_batch(4).senders is not a.senders
    ds = S.DeviceSyntheticDataset("mog_4_9", "cpu")
    g = ds.get_next_batch(16)
    assert g.nodes.shape[0] == int(g.n_node.sum()) and set(g.n_node.tolist()) <= {4, 9}
    with pytest.raises(KeyError):
        S.DeviceSyntheticDataset("moons_7", "cpu")


def test_a_graph_depends_on_its_seed_slot_and_size_only():
    spec = S.SYNTHETIC_SPECS["mom_6_10_20"]
    a = S.synthetic_batch_host(spec, [6, 10], None, 9)
    b = S.synthetic_batch_host(spec, [20, 10], None, 9)
    assert np.array_equal(a["nodes"][6:], b["nodes"][20:]) and np.array_equal(a["source"][6:], b["source"][20:])
    assert not np.array_equal(a["nodes"][6:], S.synthetic_batch_host(spec, [6, 10], None, 10)["nodes"][6:])
    mog = S.SYNTHETIC_SPECS["mog_4_9"]
    a = S.synthetic_batch_host(mog, [4, 9], [0, 1], 9)
    b = S.synthetic_batch_host(mog, [9, 9], [1, 1], 9)
    assert np.array_equal(a["nodes"][4:], b["nodes"][9:])
