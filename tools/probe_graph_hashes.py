#!/usr/bin/env python3
"""Developer probe: Weisfeiler-Lehman hashes of a batch and its uniqueness / novelty against a training set, the device route
against the route a user has without it.
  device  graph_hashes on the device edge lists (reads nothing back), uniqueness_novelty on two hash sets (reads 8 bytes: the
          count of valid graphs)
  host    senders / receivers / n_node copied to the host, one networkx.Graph per graph and
          networkx.weisfeiler_lehman_graph_hash(iterations=3) on it where networkx imports, else the numpy reference of
          tests/graph_hashes_ref.py; uniqueness / novelty from Python sets over (hash, n_node), the hashes of both sides
          already in hand - as on the device route, where the two hash sets are arguments
on
  config2   the config-2 batch (64 community_medium graphs drawn as the trainer draws them) against the training split of
            community_medium
  grid      the test split of data/grid.npz (20 graphs of up to 361 nodes) against its training split (80 graphs)
All routes run on one machine, after a warm-up, as repeated timed regions that end in a device synchronise; the routes are
alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload.  Before anything
is timed the device hashes are compared with the numpy reference for equality, and the three shares of the two routes with
each other (networkx's hash is another function, but it too is constant on isomorphism classes: the shares can differ only
where one of the two hashes collides and the other does not - the probe says so if they do).
    python tools/probe_graph_hashes.py [--repeats R]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402

from probe_graph_components import timed   # noqa: E402


def main():
    import torch
    import graph_hashes_ref as R
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.graphs import csr_of, data_dicts_to_graphs_tuple
    from gnf_amd.graph_stats import graph_hashes, uniqueness_novelty
    try:
        import networkx as nx
        host_kind = "networkx.weisfeiler_lehman_graph_hash"
    except ImportError:
        nx = None
        host_kind = "numpy reference"
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 5)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    cm = GraphDataset("graph_rnn_community_medium", 8)
    grid = GraphDataset("graph_rnn_grid", 8)
    batch_of = lambda ds, ids: data_dicts_to_graphs_tuple(ds.all.data_dicts(ids, ds._features), dev)
    workloads = {"config2": (cm.get_next_train_batch(64, dev), batch_of(cm, cm.train_ids)),
                 "grid": (batch_of(grid, grid.test_ids), batch_of(grid, grid.train_ids))}

    def host_hashes(g):
        """[(hash, n_node)] of a device batch, by way of the host"""
        n_node = g.n_node.cpu().numpy()
        s, r = g.senders.cpu().numpy().astype(np.int64), g.receivers.cpu().numpy().astype(np.int64)
        if nx is None:
            return list(zip(R.hashes(n_node, s, r, 3)["hash"].tolist(), n_node.tolist()))
        off = np.concatenate([[0], np.cumsum(n_node)])
        order = np.argsort(r, kind="stable")                         # an edge belongs to the graph of its receiver
        s, r = s[order], r[order]
        cut = np.searchsorted(r, off)
        out = []
        for k, n in enumerate(n_node.tolist()):
            x = nx.Graph()
            x.add_nodes_from(range(n))
            a, b = s[cut[k]:cut[k + 1]] - off[k], r[cut[k]:cut[k + 1]] - off[k]
            x.add_edges_from(zip(a[a != b].tolist(), b[a != b].tolist()))
            out.append((nx.weisfeiler_lehman_graph_hash(x, iterations=3), n))
        return out

    def host_shares(gen_keys, train_keys):
        known, seen, valid, distinct, novel, both = set(train_keys), set(), 0, 0, 0, 0
        for key in gen_keys:
            if key[1] == 0:
                continue
            valid += 1
            first, new = key not in seen, key not in known
            seen.add(key)
            distinct, novel, both = distinct + first, novel + new, both + (first and new)
        return [valid, distinct, novel, both]

    for name, (gen, train) in workloads.items():
        sizes, train_sizes = gen.n_node.cpu().tolist(), train.n_node.cpu().tolist()
        csr_of(gen), csr_of(train)
        d_gen, d_train = graph_hashes(gen, n_node_host=sizes), graph_hashes(train, n_node_host=train_sizes)
        for g, d in ((gen, d_gen), (train, d_train)):
            want = R.hashes(g.n_node.cpu().numpy(), g.senders.cpu().numpy(), g.receivers.cpu().numpy(), 3)
            assert np.array_equal(d["hash"].cpu().numpy(), want["hash"]), name
        u = uniqueness_novelty(d_gen, d_train)
        gen_keys, train_keys = host_hashes(gen), host_hashes(train)
        host_counts = host_shares(gen_keys, train_keys)
        row = {"workload": name, "graphs": len(sizes), "nodes": int(sum(sizes)), "edge_entries": int(gen.senders.shape[0]),
               "largest_graph": max(sizes), "training_graphs": len(train_sizes), "training_nodes": int(sum(train_sizes)),
               "training_classes": int(uniqueness_novelty(d_train, d_train)["counts"][1]),
               "counts_device": u["counts"].tolist(), "counts_host": host_counts, "host_hash": host_kind,
               "routes_agree": u["counts"].tolist() == host_counts, "repeats": repeats,
               "bytes_to_host_hashes_device_route": 0, "bytes_to_host_novelty_device_route": 8,
               "bytes_to_host_host_route": 8 * int(gen.senders.shape[0]) + 4 * len(sizes)}
        row.update(timed({"hashes_device": (lambda: graph_hashes(gen, n_node_host=sizes), 20),
                          "hashes_host": (lambda: host_hashes(gen), 1),
                          "novelty_device": (lambda: uniqueness_novelty(d_gen, d_train), 20),
                          "novelty_host": (lambda: host_shares(gen_keys, train_keys), 20)}, repeats, sync))
        row["hashes_host_over_device"] = round(row["hashes_host_ms"]["median"] / row["hashes_device_ms"]["median"], 2)
        row["novelty_host_over_device"] = round(row["novelty_host_ms"]["median"] / row["novelty_device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
