#!/usr/bin/env python3
"""Developer probe: connected components and largest-component extraction of a batch, the device route against the route a
user has without it.
  device  graph_components / keep_subgraphs("largest_component") on the device edge lists: the first reads nothing back, the
          second 16 bytes (N', E'); the kept batch comes with its CSR
  host    senders / receivers / n_node copied to the host, components there (scipy.sparse.csgraph.connected_components if scipy
          imports, else the union-find of tests/graph_components_ref.py), for the extraction the induced edge lists in numpy,
          uploaded as a new GraphsTuple whose CSR gnf_build_csr then builds
on
  config2        the config-2 batch: 64 community_medium graphs drawn as the trainer draws them
  grid_test      the test split of data/grid.npz (20 graphs of up to 361 nodes: long searches)
  config2_half   the config-2 batch with a seeded half of its undirected edges dropped: the extraction has work to do
All routes run on one machine, after a warm-up, as repeated timed regions that end in a device synchronise; the routes are
alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload.  The results of
the two routes are compared for equality before anything is timed.
    python tools/probe_graph_components.py [--repeats R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402


def timed(fns, repeats, sync):
    """fns: name -> (callable, calls per timed region); milliseconds per call"""
    out = {k: [] for k in fns}
    for k, (fn, _) in fns.items():
        fn()                       # warm-up
    sync()
    for _ in range(repeats):
        for k, (fn, calls) in fns.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            out[k].append((time.perf_counter() - t0) * 1e3 / calls)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k + "_ms": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in out.items()}


def main():
    import torch
    import graph_components_ref as R
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.graphs import GraphsTuple, clear_csr_cache, csr_of, data_dicts_to_graphs_tuple
    from gnf_amd.graph_stats import graph_components, keep_subgraphs
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        host_kind = "scipy.sparse.csgraph"
    except ImportError:
        connected_components = None
        host_kind = "numpy union-find"
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 5)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    def upload(n_node, n_edge, s, r, nodes):
        i32 = lambda v: torch.as_tensor(np.asarray(v, np.int32)).to(dev)
        return GraphsTuple(nodes=nodes, edges=torch.zeros(len(s), device=dev), receivers=i32(r), senders=i32(s),
                           globals=torch.zeros(len(n_node), device=dev), n_node=i32(n_node), n_edge=i32(n_edge))

    def halved(g, seed=2026):
        """the batch with a seeded half of its undirected edges dropped, both directions of the rest"""
        n_node = g.n_node.cpu().numpy()
        _, pairs = R._simple_pairs(n_node, g.senders.cpu().numpy(), g.receivers.cpu().numpy())
        pairs = pairs[np.random.default_rng(seed).random(len(pairs)) < 0.5]
        s, r = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
        order = np.lexsort((s, r))
        s, r = s[order], r[order]
        gid = np.searchsorted(np.cumsum(n_node), r, side="right")
        return upload(n_node, np.bincount(gid, minlength=len(n_node)), s, r, g.nodes)

    cm = GraphDataset("graph_rnn_community_medium", 8)
    grid = GraphDataset("graph_rnn_grid", 8)
    batch_of = lambda ds, ids: data_dicts_to_graphs_tuple(ds.all.data_dicts(ids, ds._features), dev)
    config2 = cm.get_next_train_batch(64, dev)
    workloads = {"config2": config2, "grid_test": batch_of(grid, grid.test_ids), "config2_half": halved(config2)}

    def host_components(g):
        n_node = g.n_node.cpu().numpy()
        s, r = g.senders.cpu().numpy().astype(np.int64), g.receivers.cpu().numpy().astype(np.int64)
        if connected_components is None:
            return n_node, s, r, R.components(n_node, s, r)["component"]
        n = int(n_node.sum())
        _, lab = connected_components(coo_matrix((np.ones(len(s), np.int8), (r, s)), shape=(n, n)), directed=False)
        first = np.full(lab.max() + 1 if n else 0, n, np.int64)
        np.minimum.at(first, lab, np.arange(n))
        return n_node, s, r, first[lab]

    def host_keep(g):
        n_node, s, r, comp = host_components(g)
        n = len(comp)
        gid = np.repeat(np.arange(len(n_node)), n_node)
        size = np.bincount(comp, minlength=n)
        best = np.zeros(len(n_node), np.int64)
        np.maximum.at(best, gid, size[comp])
        roots = np.flatnonzero((comp == np.arange(n)) & (size[comp] == best[gid]))
        root_of = np.full(len(n_node), -1, np.int64)
        root_of[gid[roots][::-1]] = roots[::-1]                     # the smallest root wins
        sub = R.subgraph(n_node, s, r, comp == root_of[gid])
        kept = upload(sub["new_n_node"], sub["n_edge"], sub["senders"], sub["receivers"],
                      g.nodes.index_select(0, torch.as_tensor(sub["node_index"]).to(dev)))
        clear_csr_cache()
        csr_of(kept)
        return sub, kept

    for name, g in workloads.items():
        sizes = g.n_node.cpu().tolist()
        csr_of(g)
        d, h = graph_components(g, n_node_host=sizes), host_components(g)[3]
        assert np.array_equal(d["component"].cpu().numpy(), h), name
        dk, (hk, _) = keep_subgraphs(g, "largest_component", n_node_host=sizes), host_keep(g)
        for k, v in (("senders", dk["graph"].senders), ("receivers", dk["graph"].receivers), ("node_index", dk["node_index"])):
            assert np.array_equal(v.cpu().numpy(), hk[k]), (name, k)
        csr_of(g)                                                   # (host_keep cleared the cache: the input's CSR again)
        row = {"workload": name, "graphs": len(sizes), "nodes": int(sum(sizes)), "edge_entries": int(g.senders.shape[0]),
               "largest_graph": max(sizes), "mean_components": round(float(d["n_components"].double().mean()), 3),
               "kept_nodes": int(dk["total_nodes"]), "kept_edge_entries": int(dk["total_edges"]), "host_components": host_kind,
               "repeats": repeats, "bytes_to_host_components_device_route": 0, "bytes_to_host_keep_device_route": 16,
               "bytes_to_host_host_route": 8 * int(g.senders.shape[0]) + 4 * len(sizes)}
        row.update(timed({"components_device": (lambda: graph_components(g, n_node_host=sizes), 20),
                          "components_host": (lambda: host_components(g), 1),
                          "keep_device": (lambda: keep_subgraphs(g, "largest_component", n_node_host=sizes), 20),
                          "keep_host": (lambda: host_keep(g), 1)}, repeats, sync))
        row["components_host_over_device"] = round(row["components_host_ms"]["median"] / row["components_device_ms"]["median"], 2)
        row["keep_host_over_device"] = round(row["keep_host_ms"]["median"] / row["keep_device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
