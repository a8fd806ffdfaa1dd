"""What a trained encoder gets wrong (the reference driver run_gnn_inference.py with its flag names, where they still mean
something): load an encoder saved by examples/run_gnn.py, run it over test batches and report, per batch, the number of wrong
edges and the quartiles of the scores of the false positives and of the false negatives - how far from the 0.5 threshold the
errors sit, which is what to look at before touching temp / shift or --tune_sigmoid.  Per graph the "complete" graph (one edge
for every pair that is a true or a predicted edge; class 1 correct, 2 false positive, 3 false negative) and the predicted graph
are collected and written to <output_file>_complete.npz / <output_file>_pred.npz.

    python examples/run_gnn.py --dataset graph_rnn_community_small --num_train_iters 200 --save_path encoder.npz
    python examples/run_gnn_inference.py --checkpoint encoder.npz --dataset graph_rnn_community_small --output_file report

Every batch is one encoder.evaluate(..., report=True): the classification, the edge lists and the order statistics are made on
the device (adj_loss.reconstruction_report); the host only slices the lists by graph.  Two departures from the reference's
figures (include/gnf_adj_report.h): the diagonal is not counted as false-positive self loops, and false negatives whose score is
exactly 0 stay in the quartiles.

The .npz files hold, over all graphs seen, n_node [G] and n_edge [G] and the concatenated per-graph edge lists senders /
receivers (graph-local ids, receivers ascending), cls (int32) and score (float32); graph g's entries are
[edge_offsets[g], edge_offsets[g + 1]).  --pickle additionally writes <output_file>_complete.p / _pred.p, lists of networkx
graphs with the class as edge weight, for the reference's visualize_graphs.py."""
import argparse
import os
import pickle
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnf_amd import adj_loss, datasets as D, encoder as E, gnn   # noqa: E402

QUARTILES = (0.0, 0.25, 0.5, 0.75, 1.0)


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True, help="a file written by encoder.save_encoder (run_gnn.py --save_path)")
    ap.add_argument("--dataset", default="graph_rnn_community")
    ap.add_argument("--train_batch_size", type=int, default=32)
    ap.add_argument("--num_train_iters", type=int, default=10)
    ap.add_argument("--node_embedding_dim", type=int, default=None, help="default: the checkpoint's")
    ap.add_argument("--gaussian_scale", type=float, default=1.0)
    ap.add_argument("--output_file", default="")
    ap.add_argument("--random_seed", type=int, default=12345)
    ap.add_argument("--pickle", action="store_true", help="also write networkx pickles, as the reference does")
    return ap


class GraphLists:
    """per-graph edge lists with graph-local ids, appended batch by batch"""

    def __init__(self):
        self.n_node, self.n_edge, self.senders, self.receivers, self.cls, self.score = [], [], [], [], [], []

    def add(self, n_node, part):
        g = part["graph"]
        n_edge = g.n_edge.cpu().numpy().astype(np.int64)
        first = np.repeat(np.concatenate([[0], np.cumsum(n_node)[:-1]]), n_edge)   # every entry's graph offset
        self.n_node.append(n_node), self.n_edge.append(n_edge)
        self.senders.append(g.senders.cpu().numpy() - first), self.receivers.append(g.receivers.cpu().numpy() - first)
        self.cls.append(part["cls"].cpu().numpy()), self.score.append(part["score"].cpu().numpy())

    def arrays(self):
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
        n_edge = cat(self.n_edge, np.int64)
        return dict(n_node=cat(self.n_node, np.int32), n_edge=n_edge.astype(np.int32),
                    edge_offsets=np.concatenate([[0], np.cumsum(n_edge)]).astype(np.int64),
                    senders=cat(self.senders, np.int32), receivers=cat(self.receivers, np.int32), cls=cat(self.cls, np.int32),
                    score=cat(self.score, np.float32))

    def networkx(self, nx):
        a, out = self.arrays(), []
        for g, n in enumerate(a["n_node"]):
            graph = nx.Graph()
            graph.add_nodes_from(range(int(n)))
            e0, e1 = a["edge_offsets"][g], a["edge_offsets"][g + 1]
            graph.add_weighted_edges_from(zip(a["senders"][e0:e1].tolist(), a["receivers"][e0:e1].tolist(),
                                              a["cls"][e0:e1].astype(np.float64).tolist()))
            out.append(graph)
        return out


def main():
    ap = make_parser()
    F = ap.parse_args()
    nx = None
    if F.pickle:
        try:
            import networkx as nx
        except ImportError:
            raise SystemExit("--pickle writes networkx graphs and networkx is not importable here; the .npz files hold the "
                             "same edge lists")
    random.seed(F.random_seed)
    np.random.seed(F.random_seed)
    torch.manual_seed(F.random_seed)
    gnn.set_random_seed(F.random_seed)
    dev = torch.device("cuda", 0)
    enc, hp = E.load_encoder(F.checkpoint)
    dim = int(hp["node_dim"])
    if F.node_embedding_dim is not None and F.node_embedding_dim != dim:
        ap.error(f"--node_embedding_dim {F.node_embedding_dim}: the checkpoint's encoder reads {dim} features per node")
    dist_fn = E.distance_of(hp)
    dataset = D.GraphDataset(F.dataset, dim, F.gaussian_scale, seed=F.random_seed)
    complete, pred = GraphLists(), GraphLists()
    for i in range(F.num_train_iters):
        batch = dataset.get_next_test_batch(F.train_batch_size, dev)
        ev = E.evaluate(enc, batch, distance_fn=dist_fn, report={"quantiles": QUARTILES})
        rep = ev["report"]
        print(f"iteration num {i}")
        print(f"total_incorrect_edges {float(ev['total_incorrect_edges'])}")
        if int(rep["fp_count"]) > 0:
            print(f"false positive quartiles: {rep['fp_quantiles'].cpu().numpy()}")
        if int(rep["fn_count"]) > 0:
            print(f"false negative quartiles: {rep['fn_quantiles'].cpu().numpy()}")
        n_node = batch.n_node.cpu().numpy().astype(np.int64)
        complete.add(n_node, rep)
        pred.add(n_node, adj_loss.predicted_graph(rep))
    for name, lists in (("complete", complete), ("pred", pred)):
        np.savez(f"{F.output_file}_{name}.npz", **lists.arrays())
        if nx is not None:
            with open(f"{F.output_file}_{name}.p", "wb") as f:
                pickle.dump(lists.networkx(nx), f)
    total = complete.arrays()
    print(f"{len(total['n_node'])} graphs, {len(total['cls'])} listed pairs "
          f"({int((total['cls'] == 1).sum())} correct, {int((total['cls'] == 2).sum())} false positive, "
          f"{int((total['cls'] == 3).sum())} false negative) written to {F.output_file}_complete.npz / {F.output_file}_pred.npz")


if __name__ == "__main__":
    main()
