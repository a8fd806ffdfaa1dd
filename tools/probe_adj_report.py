#!/usr/bin/env python3
"""Developer probe: the reconstruction report, the device route against the host route the reference takes
(run_gnn_inference.py:107-163).
  device  adj_loss.reconstruction_report (gnf_adj_report_count_f32 / _fill / gnf_score_select_f32): classified edge list with
          scores, class counts and the quartiles of the false positives' and false negatives' scores, batch-wide; exact-size
          mode (one 8-byte read of the entry total), and with an edge capacity (nothing read on the host)
  host    flow.pred_adj for the per-graph probability blocks -> host, a dense true adjacency per graph from the host edge
          list, numpy classification (threshold, correct / false positive / false negative, the class-weighted complete
          matrix and np.nonzero for the edge lists) and np.quantile over the two classes' scores
on
  config2   the config-2 batch: 64 community_medium graphs drawn as the trainer draws them, D = 64
  grid32    32 graphs of the grid data set, D = 64 (about 1.45 M ordered pairs)
Embeddings: N(0, 1) * 0.5 * D^-1/4 with one row in eight stretched by 4 (the tests' distribution: every class occurs).
Before anything is timed the two routes are compared: class counts equal, quartiles equal to np.quantile's within the bound
tests/test_adj_report_cpu.py derives.  Both routes run on one machine, after a warm-up, as repeated timed regions that end in a
device synchronise; the routes alternate inside every repeat; median, min and max go out as one JSON line per workload
(DESIGN.md section 9.16).
    python tools/probe_adj_report.py [--repeats R] > profiles/adj_report_probe.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUARTILES = (0.0, 0.25, 0.5, 0.75, 1.0)


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
    import numpy as np
    import torch
    from gnf_amd.adj_loss import reconstruction_report
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.flow import pred_adj
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 5)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    gen = torch.Generator(device="cpu").manual_seed(0)

    def embed(g, d):
        n = int(g.nodes.shape[0])
        z = torch.randn(n, d, generator=gen) * 0.5 * d ** -0.25
        z[torch.rand(n, generator=gen) < 0.125] *= 4.0
        return g.replace(nodes=z.to(dev))

    workloads = {"config2": (GraphDataset("graph_rnn_community_medium", 8).get_next_train_batch(64, dev), 20),
                 "grid32": (GraphDataset("graph_rnn_grid", 8).get_next_train_batch(32, dev), 5)}
    for name, (true, calls) in workloads.items():
        emb = embed(true, 64)
        sizes = true.n_node.cpu().tolist()
        off = np.concatenate([[0], np.cumsum(sizes)])
        snd, rcv = true.senders.cpu().numpy().astype(np.int64), true.receivers.cpu().numpy().astype(np.int64)

        def host():
            blocks = [b.cpu().numpy() for b in pred_adj(emb)]
            fp_scores, fn_scores, lists, counts = [], [], [], np.zeros(3, np.int64)
            gid = np.searchsorted(off, snd, side="right") - 1
            for g, p in enumerate(blocks):
                ng = sizes[g]
                m = gid == g
                a = np.zeros((ng, ng), bool)
                a[rcv[m] - off[g], snd[m] - off[g]] = True      # [receiver, sender], as the blocks
                np.fill_diagonal(a, False)
                pred = p > 0.5
                correct, fp, fn = pred & a, pred & ~a, a & ~pred
                complete = correct + 2 * fp + 3 * fn
                r, s = np.nonzero(complete)
                lists.append((s, r, complete[r, s], p[r, s]))
                fp_scores.append(p[fp]), fn_scores.append(p[fn])
                counts += (int(correct.sum()), int(fp.sum()), int(fn.sum()))
            fps, fns_ = np.concatenate(fp_scores).astype(np.float64), np.concatenate(fn_scores).astype(np.float64)
            return counts, np.quantile(fps, QUARTILES), np.quantile(fns_, QUARTILES), lists

        rep = reconstruction_report(emb, true, n_node_host=sizes)
        counts, fpq, fnq, _ = host()
        total = int(rep["totals"][0])
        row = {"measurement": "reconstruction_report", "workload": name, "graphs": len(sizes), "nodes": int(off[-1]), "D": 64,
               "largest_graph": max(sizes), "ordered_pairs": int(sum(s * s - s for s in sizes)), "entries": total,
               "class_pairs": [int(v) for v in rep["totals"][1:]], "repeats": repeats, "calls_per_region": calls}
        assert row["class_pairs"] == counts.tolist(), (row, counts)          # the same arithmetic as pred_adj: equal
        for got, want in ((rep["fp_quantiles"], fpq), (rep["fn_quantiles"], fnq)):
            assert np.abs(got.cpu().numpy() - want).max() <= 8.0 * 2.0 ** -53, (got, want)   # both float64 on scores <= 1
        row["fp_quartiles"] = [float(v) for v in rep["fp_quantiles"]]
        row["fn_quartiles"] = [float(v) for v in rep["fn_quantiles"]]
        row.update(timed({"device": (lambda: reconstruction_report(emb, true, n_node_host=sizes), calls),
                          "device_capacity": (lambda: reconstruction_report(emb, true, n_node_host=sizes, edge_capacity=total),
                                              calls),
                          "host": (host, max(calls // 5, 1))}, repeats, sync))
        row["host_over_device"] = round(row["host_ms"]["median"] / row["device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
