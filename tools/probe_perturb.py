#!/usr/bin/env python3
"""Developer probe: one ready noisy batch - edge list on the device, both CSRs available - from a true batch that is already
on the device, by the host route and by the device route (include/gnf_perturb.h), same batch, same seed.
  host    edge list to the host, datasets.perturb_keep_mask in numpy, upload of the surviving list and its n_edge,
          build_csr_device twice
  device  datasets.perturb_batch: one gnf_perturb_edges (the true batch's CSRs are cache hits), one 8-byte read of E'
  capture datasets.perturb_batch(exact=False): the same call without the read (what a captured step would replay)
Shapes: the two of tools/probe_batches.py
  cm64            64 x community_medium (DeviceGraphDataset.batch_of)
  grid32_complete 32 x grid node counts, complete topology (datasets.complete_batch), 1.45 M edges
After a warm-up, `repeats` timed regions per route, the routes alternating inside every repeat; a region is `calls` calls
between two device events on the current stream (the host route's copies and numpy work lie between them too, so its figure
is the time the stream waits for a ready batch).  Before anything is timed the routes' arrays are compared for equality.
Median and min .. max go out as one JSON line per shape, with the bytes the device route moves computed from the shapes
(DESIGN.md section 9.13).
    python tools/probe_perturb.py [--repeats R] [--shapes a,b] > profiles/perturb_probe.jsonl"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def model_bytes(b, n, e, kept):
    """bytes gnf_perturb_edges reads and writes, from the shapes: pass 1 reads the 4 edge arrays and writes 3 W words; the scan
    reads them twice and n_edge twice and writes the bases; pass 3 reads a word and a base per entry-wave, reads and writes the
    survivors of the 4 edge arrays, reads both rowptrs with a word and a base each and writes them, and per graph two segment
    starts, two words and bases and two counts (the row searches of pass 1 hit the cache and are not counted)"""
    w = (e + 63) // 64
    mark = 4 * e * 4 + 3 * w * 8
    scan = 2 * 3 * w * 8 + 2 * b * 4 + 3 * (w + 1) * 4 + (b + 1) * 4 + 16
    fill = 3 * w * 12 + 2 * 4 * kept * 4 + 2 * (n + 1) * (4 + 12 + 4) + b * (8 + 24 + 8)
    return mark + scan + fill


def main():
    import torch
    from gnf_amd import datasets as D
    from gnf_amd.graphs import GraphsTuple, build_csr_device, csr_of
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    repeats = int(arg("--repeats", 9))
    shapes = arg("--shapes", "cm64,grid32_complete").split(",")
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    p, seed = 0.3, 12345

    def true_batch(name):
        if name == "cm64":
            ds = D.DeviceGraphDataset("graph_rnn_community_medium", 64, device=dev)
            return ds.batch_of(D.GraphDataset("graph_rnn_community_medium", 64).sample_ids(64)), 20
        sizes = D.GraphDataset("graph_rnn_grid", 1).all.n_node[:32].astype(np.int32)
        return D.complete_batch(torch.zeros(int(sizes.sum()), 8, device=dev), sizes, dev), 5

    def host_route(true):
        s, r = true.senders.cpu().numpy(), true.receivers.cpu().numpy()
        n_edge = true.n_edge.cpu().numpy().astype(np.int64)
        keep = D.perturb_keep_mask(s, r, p, seed)
        kept = np.bincount(np.repeat(np.arange(len(n_edge)), n_edge)[keep], minlength=len(n_edge)).astype(np.int32)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        e2 = int(keep.sum())
        g = GraphsTuple(nodes=true.nodes, edges=torch.zeros(e2, device=dev), receivers=up(r[keep]), senders=up(s[keep]),
                        globals=true.globals, n_node=true.n_node, n_edge=up(kept))
        return g, build_csr_device(g), build_csr_device(g, by_sender=True)

    def device_route(true):
        g, _ = D.perturb_batch(true, p, seed)
        return g, csr_of(g), csr_of(g, by_sender=True)

    def timed(fns, calls):
        out = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                b.synchronize()
                out[k].append(a.elapsed_time(b) / calls)
        med = lambda v: sorted(v)[len(v) // 2]
        return {k + "_ms": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in out.items()}

    for name in shapes:
        true, calls = true_batch(name)
        csr_of(true), csr_of(true, by_sender=True)
        (ga, ca, ta), (gb, cb, tb) = host_route(true), device_route(true)
        e2 = int(gb.senders.shape[0])
        agree = all(torch.equal(getattr(ga, k), getattr(gb, k)) for k in ("senders", "receivers", "n_edge"))
        agree = agree and torch.equal(ca.rowptr, cb.rowptr) and torch.equal(ta.rowptr, tb.rowptr)
        agree = bool(agree and torch.equal(ca.col[:e2], cb.col[:e2]) and torch.equal(ta.col[:e2], tb.col[:e2]))
        b, n, e = int(true.n_node.shape[0]), int(true.nodes.shape[0]), int(true.senders.shape[0])
        row = {"shape": name, "graphs": b, "nodes": n, "edges": e, "edges_kept": e2, "deletion_prob": p, "routes_agree": agree,
               "repeats": repeats, "calls_per_region": calls, "device_route_model_bytes": model_bytes(b, n, e, e2)}
        assert agree, name
        del ga, ca, ta, gb, cb, tb
        row.update(timed({"ready_host": lambda: host_route(true), "ready_device": lambda: device_route(true),
                          "ready_device_no_read": lambda: D.perturb_batch(true, p, seed, exact=False)}, calls))
        row["host_over_device"] = round(row["ready_host_ms"]["median"] / row["ready_device_ms"]["median"], 2)
        row["model_gb_per_s_no_read"] = round(row["device_route_model_bytes"] / row["ready_device_no_read_ms"]["median"] / 1e6, 1)
        print(json.dumps(row), flush=True)
        del true
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
