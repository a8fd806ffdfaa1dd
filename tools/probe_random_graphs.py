#!/usr/bin/env python3
"""Developer probe: from "want a batch of random graphs" to "edge list and both CSRs ready on the device", by the host route
and by the device route (include/gnf_random_graphs.h), in one process.
  host    random_graphs.random_graphs_host (the numpy twin) + the upload of the index arrays + csr_of twice: gnf_build_csr by
          receiver and by sender
  device  random_graphs.erdos_renyi / barabasi_albert in exact-size mode (one 8-byte read of the edge total) + csr_of twice
          (cache hits)
Shapes: 64 graphs of the first 64 sizes of community_medium, and 32 graphs of 361 nodes (the size of a 19 x 19 grid); each for
G(n, p) at the fitted density and for Barabasi-Albert at the fitted m (fit_params on the data set's own edge counts; a 19 x 19
grid has 684 edges).
After a warm-up, `repeats` timed regions per route, the routes alternating inside every repeat; a region is `calls` batches
between two readings of the host clock, the second after a device synchronise, so host work counts - it is what the host route
consists of.  Median and min .. max go out as one JSON line per measurement.
    python tools/probe_random_graphs.py [--repeats R] [--calls C] > profiles/random_graphs_probe.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def main():
    import torch
    from gnf_amd import random_graphs as G
    from gnf_amd.graphs import GraphsTuple, csr_of
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    repeats, calls = int(arg("--repeats", 5)), int(arg("--calls", 4))
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    seed = 12345

    def timed(fns, warm):
        out = {k: [] for k in fns}
        for fn in fns.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e3 / calls)
        med = lambda v: sorted(v)[len(v) // 2]
        return {k + "_ms": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in out.items()}

    def ready(graph):
        return graph, csr_of(graph), csr_of(graph, by_sender=True)

    def host_route(model, sizes, par):
        h = G.random_graphs_host(model, sizes, par, seed=seed)
        up = lambda a: torch.from_numpy(a).to(dev)
        e, b, n = h["total"], len(sizes), int(sum(sizes))
        return ready(GraphsTuple(nodes=torch.zeros(n, 1, device=dev), edges=torch.zeros(e, device=dev), receivers=up(h["receivers"]),
                                 senders=up(h["senders"]), globals=torch.zeros(b, device=dev), n_node=up(h["n_node"]),
                                 n_edge=up(h["n_edge"])))

    d = np.load(os.path.join(ROOT, "data", "community_medium.npz"))
    # (the data sets store both directions and one loop per node)
    shapes = {"community_medium_64": (d["n_node"][:64].astype(np.int64), (d["n_edge"][:64].astype(np.int64) - d["n_node"][:64]) // 2),
              "grid_19x19_32": (np.full(32, 361, np.int64), np.full(32, 684, np.int64))}
    for name, (sizes, edges) in shapes.items():
        p = G.fit_params(torch.from_numpy(edges), torch.from_numpy(sizes), "erdos_renyi").numpy()
        m = G.fit_params(torch.from_numpy(edges), torch.from_numpy(sizes), "barabasi_albert").numpy()
        sizes = sizes.tolist()
        for model, make, par, host_par in (("erdos_renyi", G.erdos_renyi, p, G.thresholds(p, len(sizes))),
                                           ("barabasi_albert", G.barabasi_albert, m, m)):
            g, _, _ = ready(make(sizes, par, seed=seed, device=dev)["graph"])
            row = {"measurement": "ready_random_graphs", "shape": name, "model": model, "graphs": len(sizes), "nodes": int(sum(sizes)),
                   "edges": int(g.senders.shape[0]), "repeats": repeats, "calls_per_region": calls}
            row.update(timed({"ready_host": lambda: host_route(model, sizes, host_par),
                              "ready_device": lambda: ready(make(sizes, par, seed=seed, device=dev)["graph"])}, 2))
            row["host_over_device"] = round(row["ready_host_ms"]["median"] / row["ready_device_ms"]["median"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
