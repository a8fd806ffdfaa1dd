#!/usr/bin/env python3
"""Developer probe: Laplacian spectra of generated graphs, the device route against the route a user has without it.
  device  graph_spectra (gnf_graph_spectra on the device edge lists): nothing reaches the host
  host    senders / receivers / n_node copied to the host, then per graph the dense normalised Laplacian,
          numpy.linalg.eigvalsh (LAPACK) and the clamped histogram - tests/graph_spectra_ref.py
on
  config2    the config-2 batch: 64 community_medium graphs drawn as the trainer draws them (at most 60 nodes: LDS route)
  grid_test  the test split of data/grid.npz (20 graphs of 120 .. 361 nodes: workspace route)
All routes run on one machine, after a warm-up, as repeated timed regions (20 device calls, one host call) that end in a
device synchronise; the routes are alternated inside every repeat and median, min and max over the repeats go out as one
JSON line per workload.  The eigenvalues and histograms of the two routes are compared before anything is timed.
    python tools/probe_graph_spectra.py [--repeats R]"""
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
    import graph_spectra_ref as R
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    from gnf_amd.graph_stats import SPECTRA_LDS_NODES, graph_spectra
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 5)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    cm = GraphDataset("graph_rnn_community_medium", 8)
    grid = GraphDataset("graph_rnn_grid", 8)
    batch_of = lambda ds, ids: data_dicts_to_graphs_tuple(ds.all.data_dicts(ids, ds._features), dev)
    workloads = {"config2": cm.get_next_train_batch(64, dev), "grid_test": batch_of(grid, grid.test_ids)}

    def host_route(g):
        n_node = g.n_node.cpu().numpy()
        s, r = g.senders.cpu().numpy().astype(np.int64), g.receivers.cpu().numpy().astype(np.int64)
        return R.graph_spectra(n_node, s, r)

    for name, g in workloads.items():
        sizes = g.n_node.cpu().tolist()
        dev_out, host_out = graph_spectra(g, n_node_host=sizes), host_route(g)
        err = float(np.abs(dev_out["eigenvalues"].cpu().numpy() - host_out["eigenvalues"]).max())
        # (a grid is bipartite and full of repeated eigenvalues, some on bin edges: only counts next to an edge may differ)
        moved = int(np.abs(dev_out["spectral_hist"].cpu().numpy() - host_out["spectral_hist"]).sum()) // 2
        assert err <= 1e-11, (name, err)
        row = {"workload": name, "graphs": len(sizes), "nodes": int(sum(sizes)), "edge_entries": int(g.senders.shape[0]),
               "largest_graph": max(sizes), "route": "lds" if max(sizes) <= SPECTRA_LDS_NODES else "workspace",
               "max_abs_eigenvalue_error": err, "counts_in_another_bin": moved, "repeats": repeats,
               "bytes_to_host_device_route": 0, "bytes_to_host_host_route": 8 * int(g.senders.shape[0]) + 4 * len(sizes)}
        row.update(timed({"device": (lambda: graph_spectra(g, n_node_host=sizes), 20),
                          "host": (lambda: host_route(g), 1)}, repeats, sync))
        row["host_over_device"] = round(row["host_ms"]["median"] / row["device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
