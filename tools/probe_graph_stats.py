#!/usr/bin/env python3
"""Developer probe: scoring generated graphs, the device route against the route a user has without it.
  device  graph_stats (gnf_graph_stats on the device edge lists) and hist_mmd (gnf_hist_mmd_f64); only the two counts
          hist_mmd checks and the final scalar reach the host
  host    senders / receivers / n_node copied to the host, one graph at a time through networkx (dense numpy when networkx
          is not importable): degree histogram and 100-bin clustering histogram; then a Python loop over all histogram pairs
          with the cumulative-sum EMD and the Gaussian kernel - GraphRNN-style evaluation with its EMD solver replaced by
          the closed form (so the host side is, if anything, flattered)
on
  config2    the config-2 batch: 64 community_medium graphs drawn as the trainer draws them
  grid_test  the test split of data/grid.npz (20 graphs of 120 .. 361 nodes)
  mmd        degree and clustering MMD^2 of --mmd-graphs (default 256) community_medium graphs per side, train against test
Both routes run on one machine, after a warm-up, as repeated timed regions (50 / 10 device calls, one host call) that end
in a device synchronise; the two routes
are alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload, with the
bytes each route moves across the host link.  The statistics are compared before anything is timed.
    python tools/probe_graph_stats.py [--repeats R] [--mmd-graphs G]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def host_stats(n_node, senders, receivers, bins=100):
    """Per-graph degree histograms (lists) and clustering histograms on the host."""
    try:
        import networkx as nx
    except ImportError:
        nx = None
    noff = np.concatenate([[0], np.cumsum(n_node)])
    order = np.argsort(receivers, kind="stable")
    s, r = senders[order], receivers[order]
    cut = np.searchsorted(r, noff)
    deg_h, clu_h = [], []
    for g, n in enumerate(n_node):
        n, n0 = int(n), int(noff[g])
        ls, lr = s[cut[g]:cut[g + 1]] - n0, r[cut[g]:cut[g + 1]] - n0
        if nx is not None:
            gr = nx.Graph()
            gr.add_nodes_from(range(n))
            gr.add_edges_from(zip(ls.tolist(), lr.tolist()))
            gr.remove_edges_from(nx.selfloop_edges(gr))
            deg_h.append(np.asarray(nx.degree_histogram(gr)))
            c = np.asarray(list(nx.clustering(gr).values()), np.float64)
        else:
            a = np.zeros((n, n), bool)
            a[lr, ls] = True
            a |= a.T
            a[np.arange(n), np.arange(n)] = False
            m = a.astype(np.int64)
            d = m.sum(1)
            t = np.einsum("ij,ji->i", m @ m, m) // 2
            deg_h.append(np.bincount(d, minlength=1))
            c = np.where(d >= 2, 2.0 * t / np.maximum(d * (d - 1), 1), 0.0)
        clu_h.append(np.histogram(c, bins=bins, range=(0.0, 1.0))[0])
    return deg_h, clu_h


def host_mmd(ha, hb, sigma, scaling):
    width = max(max(len(h) for h in ha), max(len(h) for h in hb))
    pm = []
    for hs in (ha, hb):
        rows = []
        for h in hs:
            p = np.zeros(width)
            p[:len(h)] = h
            if p.sum() > 0:
                rows.append(p / p.sum())
        pm.append(rows)

    def block(u, v):
        tot = 0.0
        for x in u:
            for y in v:
                w = np.abs(np.cumsum(x - y)[:-1]).sum() / scaling
                tot += np.exp(-w * w / (2.0 * sigma * sigma))
        return tot / (len(u) * len(v))
    return block(pm[0], pm[0]) + block(pm[1], pm[1]) - 2.0 * block(pm[0], pm[1])


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
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    from gnf_amd.graph_stats import graph_stats, hist_mmd
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats, mmd_graphs = arg("--repeats", 7), arg("--mmd-graphs", 256)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    cm = GraphDataset("graph_rnn_community_medium", 8)
    grid = GraphDataset("graph_rnn_grid", 8)
    batch_of = lambda ds, ids: data_dicts_to_graphs_tuple(ds.all.data_dicts(ids, ds._features), dev)
    workloads = {"config2": cm.get_next_train_batch(64, dev), "grid_test": batch_of(grid, grid.test_ids)}

    def to_host(g):
        return g.n_node.cpu().numpy(), g.senders.cpu().numpy().astype(np.int64), g.receivers.cpu().numpy().astype(np.int64)

    for name, g in workloads.items():
        sizes = g.n_node.cpu().tolist()
        st = graph_stats(g, n_node_host=sizes)
        deg_h, clu_h = host_stats(*to_host(g))
        dh = st["degree_hist"].cpu().numpy()
        for i, h in enumerate(deg_h):
            assert (dh[i, :len(h)] == h).all() and dh[i, len(h):].sum() == 0, (name, i)
        # (numpy.histogram rounds bin edges in floating point: the clustering histograms may differ on an exact edge)
        moved = int(np.abs(st["clustering_hist"].cpu().numpy() - np.asarray(clu_h)).sum()) // 2
        row = {"workload": name, "graphs": len(sizes), "nodes": int(sum(sizes)), "edge_entries": int(g.senders.shape[0]),
               "largest_graph": max(sizes), "repeats": repeats, "clustering_nodes_on_another_edge_side": moved,
               "bytes_to_host_device_route": 0, "bytes_to_host_host_route": 8 * int(g.senders.shape[0]) + 4 * len(sizes)}
        row.update(timed({"device": (lambda: graph_stats(g, n_node_host=sizes), 50),
                          "host": (lambda: host_stats(*to_host(g)), 1)}, repeats, sync))
        print(json.dumps(row), flush=True)

    sets = [batch_of(cm, cm.rng.choice(ids, size=mmd_graphs, replace=True)) for ids in (cm.train_ids, cm.test_ids)]
    stats = [graph_stats(g) for g in sets]
    hosts = [host_stats(*to_host(g)) for g in sets]

    def device_mmd():
        return (float(hist_mmd(stats[0]["degree_hist"], stats[1]["degree_hist"], "gaussian_emd", 1.0, 1.0)),
                float(hist_mmd(stats[0]["clustering_hist"], stats[1]["clustering_hist"], "gaussian_emd", 0.1, 100.0)))

    def host_mmd_both():
        return (host_mmd(hosts[0][0], hosts[1][0], 1.0, 1.0), host_mmd(hosts[0][1], hosts[1][1], 0.1, 100.0))

    d, h = device_mmd(), host_mmd_both()
    assert abs(d[0] - h[0]) <= 1e-10, (d, h)
    row = {"workload": "mmd", "graphs_per_side": mmd_graphs, "degree_bins": int(stats[0]["degree_hist"].shape[1]),
           "clustering_bins": 100, "pairs": (2 * mmd_graphs) * (2 * mmd_graphs + 1) // 2, "repeats": min(repeats, 3),
           "degree_mmd": d[0], "clustering_mmd_device": d[1], "clustering_mmd_host": h[1],
           "bytes_to_host_device_route": 2 * (16 + 8), "bytes_to_host_host_route": "as the statistics' host route, per side"}
    row.update(timed({"device": (device_mmd, 10), "host": (host_mmd_both, 1)}, min(repeats, 3), sync))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
