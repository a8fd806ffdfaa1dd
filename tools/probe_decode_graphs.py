#!/usr/bin/env python3
"""Developer probe: sampled embeddings -> edge lists + CSR, flow.decode_graphs against the route the code had before it:
  decode   flow.decode_graphs (gnf_adj_edges_count_f32, one 8-byte read of the total, gnf_adj_edges_fill; CSR comes with it)
  parent   flow.pred_adj -> `> 0.5` -> torch.nonzero per block -> int32 edge lists -> gnf_build_csr (by receiver)
on two batches:
  driver   the data driver's sampling batch at its default flags: 8 graphs of 8 .. 19 nodes, D = 200
  config4  256 graphs of 100 .. 500 nodes, D = 64 (the config-4 stand-in's sizes)
Both routes end with the edge lists and the CSR on the device and are checked to agree before anything is timed.  Both
synchronise with the host by construction (the parent once per graph), so whole calls are timed with the host clock between
device synchronisations.  The two routes are ALTERNATED inside every repeat (other work shares the machine: a difference is
judged against the spread of the repeats); median and min .. max over the repeats go out as one JSON line per batch, with
the bytes each route writes to device memory.  Every measurement round runs in a child process under a time limit of its
own, and the probe ends at the first one that fails.
    python tools/probe_decode_graphs.py [--repeats R] [--iters K]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batches():
    import numpy as np
    rng = np.random.default_rng(12345)
    out = {}
    n_node = rng.integers(8, 20, size=8).astype(np.int32)           # examples/train_grevnet_with_data.py: make_chunks sizes
    rows = []
    for n in n_node:
        centres = rng.standard_normal((2, 200)) * 0.6
        rows.append(centres[rng.integers(0, 2, size=n)] + 0.1 * rng.standard_normal((n, 200)))
    out["driver"] = (n_node, np.concatenate(rows).astype(np.float32))
    n_node = rng.integers(100, 501, size=256).astype(np.int32)
    out["config4"] = (n_node, (0.6 * 64 ** -0.25 * rng.standard_normal((int(n_node.sum()), 64))).astype(np.float32))
    return out


def child(iters):
    import numpy as np
    import torch
    from gnf_amd import _abi
    from gnf_amd.flow import decode_graphs, pred_adj
    from gnf_amd.graphs import GraphsTuple, build_csr_device
    dev = torch.device("cuda:0")
    lib = _abi.lib()
    res = {}
    for name, (n_node, z) in batches().items():
        b, n = len(n_node), int(n_node.sum())
        g = GraphsTuple(nodes=torch.as_tensor(z).to(dev), edges=torch.zeros(0, device=dev),
                        receivers=torch.zeros(0, dtype=torch.int32, device=dev), senders=torch.zeros(0, dtype=torch.int32, device=dev),
                        globals=torch.zeros(b, device=dev), n_node=torch.as_tensor(n_node).to(dev),
                        n_edge=torch.zeros(b, dtype=torch.int32, device=dev))
        sizes = n_node.tolist()

        def decode():
            return decode_graphs(g, n_node_host=sizes)

        def parent():
            s, r, ne, off = [], [], [], 0
            for blk, k in zip(pred_adj(g), sizes):
                idx = torch.nonzero(blk > 0.5)
                r.append(idx[:, 0] + off), s.append(idx[:, 1] + off), ne.append(idx.shape[0])
                off += k
            gg = g.replace(senders=torch.cat(s).to(torch.int32), receivers=torch.cat(r).to(torch.int32),
                           n_edge=torch.tensor(ne, dtype=torch.int32, device=dev))
            return gg, build_csr_device(gg)

        a, (pg, pcsr) = decode(), parent()
        e = int(a["total_edges"])
        assert torch.equal(a["graph"].senders, pg.senders) and torch.equal(a["graph"].receivers, pg.receivers)
        assert torch.equal(a["csr"].rowptr, pcsr.rowptr) and torch.equal(a["csr"].col, pcsr.col[:e])
        fns = {"decode": decode, "parent": parent}
        for fn in fns.values():   # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {}
        for fname, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            t[fname] = (time.perf_counter() - t0) * 1e3 / iters
        n2 = int((n_node.astype(np.int64) ** 2).sum())
        ws = int(lib.gnf_adj_edges_workspace_bytes(b, n, int(n_node.max())))
        t["bytes_decode"] = ws + 4 * (n + 1) + 4 * b + 8 + 8 * e          # workspace, rowptr, n_edge, total, senders + receivers
        t["bytes_parent"] = 4 * n2 + n2 + 16 * e + 8 * e + 4 * (n + 1) + 4 * e   # blocks, masks, nonzero's int64 pairs, int32 lists, CSR
        t.update(nodes=n, graphs=b, edges=e, sum_n2=n2)
        res[name] = t
    print(json.dumps(res), flush=True)


def main():
    if "--child" in sys.argv:
        return child(int(sys.argv[sys.argv.index("--child") + 1]))
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    rows = []
    for _ in range(repeats):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(iters)], capture_output=True, text=True,
                             timeout=240)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"probe_decode_graphs: a measurement round failed with status {res.returncode}; stopping")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    for name in rows[0]:
        first = rows[0][name]
        out = {"batch": name, "repeats": repeats, "iters": iters}
        out.update({k: first[k] for k in ("nodes", "graphs", "edges", "sum_n2", "bytes_decode", "bytes_parent")})
        for fn in ("decode", "parent"):
            v = [row[name][fn] for row in rows]
            out[fn + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["parent_over_decode"] = round(med([row[name]["parent"] / row[name]["decode"] for row in rows]), 2)
        out["bytes_parent_over_decode"] = round(first["bytes_parent"] / first["bytes_decode"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
