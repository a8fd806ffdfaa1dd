"""Float64 reference of the per-graph log-likelihood terms (gnf_grevnet_per_graph_f32, flow.log_prob_per_graph).

A batch is a block-diagonal union of graphs and log|det| is a plain sum over nodes, so graph g's share is the sum of s over
ITS rows (every half-step, every feature) plus, per batch-norm bijector, n_g times the per-node term ildj / N - with the
moments of the whole batch.  `PerGraphDense` repeats the loop of the oracle's Fp64Dense.f (same gnn, bn_inverse, _net)
and keeps s.sum(axis=1) per node and each bijector's ildj / N; `PerGraphGraphAttn` does the same on top of the dense
graph-scope attention reference of graph_attn_ref.py.  The committed oracle is not edited."""
import numpy as np

from oracle import gnf_oracle as O

import graph_attn_ref as R

LN_2PI = O.LN_2PI


def graph_ids(n_node):
    n_node = np.asarray(n_node, np.int64)
    return np.repeat(np.arange(len(n_node)), n_node)


def sum_by_graph(per_node, n_node):
    """[N] -> [B]; an empty graph gets 0"""
    out = np.zeros(len(n_node), np.float64)
    np.add.at(out, graph_ids(n_node), np.asarray(per_node, np.float64))
    return out


def assemble(z, row_logdet, c_total, n_node):
    """the [B] vectors flow.log_prob_per_graph returns, from z [N, D], the per-node log-det and the bijectors' summed c"""
    z = np.asarray(z, np.float64)
    n_node = np.asarray(n_node, np.int64)
    d = z.shape[1]
    num = n_node.astype(np.float64)
    logdet = sum_by_graph(row_logdet, n_node) + num * c_total
    sumsq = sum_by_graph((z * z).sum(axis=1), n_node)
    zs = -0.5 * sumsq - 0.5 * d * LN_2PI * num
    xs = zs + logdet
    return {"z": z, "log_det_jacobian": logdet, "sumsq": sumsq, "log_prob_zs": zs, "log_prob_xs": xs, "num_nodes": num,
            "log_prob_xs_per_node": xs / np.maximum(num, 1.0), "row_logdet": np.asarray(row_logdet, np.float64),
            "c_total": float(c_total)}


class PerGraphDense(O.Fp64Dense):
    """Fp64Dense whose f keeps the per-node log-det (same loop, same gnn / bn_inverse / _net)."""

    def f_rows(self, x, params, num_timesteps, weight_sharing=False):
        """-> (z [N, D], per-node sum of s over all half-steps [N], sum over the bijectors of ildj / N)"""
        x = np.asarray(x, np.float64)
        hdim = x.shape[1] // 2
        x0, x1 = x[:, :hdim].copy(), x[:, hdim:].copy()
        rows = np.zeros(x.shape[0], np.float64)
        c_total = 0.0
        bns = params.get("bn")
        for i in range(num_timesteps):
            if bns is not None:
                x0, ildj, _, _ = self.bn_inverse(x0, bns[0][i])
                c_total += ildj / x.shape[0]
            s = self.gnn(x0, O._net(params, "s", 0, i, weight_sharing))
            t = self.gnn(x0, O._net(params, "t", 0, i, weight_sharing))
            rows += s.sum(axis=1)
            x1 = x1 * np.exp(s) + t
            if bns is not None:
                x1, ildj, _, _ = self.bn_inverse(x1, bns[1][i])
                c_total += ildj / x.shape[0]
            s = self.gnn(x1, O._net(params, "s", 1, i, weight_sharing))
            t = self.gnn(x1, O._net(params, "t", 1, i, weight_sharing))
            rows += s.sum(axis=1)
            x0 = x0 * np.exp(s) + t
        return np.concatenate([x0, x1], axis=1), rows, c_total

    def per_graph_terms(self, x, params, num_timesteps, n_node, weight_sharing=False):
        z, rows, c = self.f_rows(x, params, num_timesteps, weight_sharing)
        return assemble(z, rows, c, n_node)


class PerGraphGraphAttn(R.GraphAttnGather):
    """The dense graph-scope attention reference (float64 torch) with the same bookkeeping."""

    def f_rows(self, x, params, num_timesteps, weight_sharing=False):
        torch = self.torch
        self._mlp_calls = -1
        hdim = x.shape[1] // 2
        x0, x1 = x[:, :hdim], x[:, hdim:]
        rows = torch.zeros(x.shape[0], dtype=self.dtype)
        c_total = 0.0
        bns = params.get("bn")
        for i in range(num_timesteps):
            if bns is not None:
                x0, ildj = self.bn_inverse(x0, bns[0][i])
                c_total += float(ildj) / x.shape[0]
            s = self.gnn(x0, O._net(params, "s", 0, i, weight_sharing))
            t = self.gnn(x0, O._net(params, "t", 0, i, weight_sharing))
            rows = rows + s.sum(dim=1)
            x1 = x1 * torch.exp(s) + t
            if bns is not None:
                x1, ildj = self.bn_inverse(x1, bns[1][i])
                c_total += float(ildj) / x.shape[0]
            s = self.gnn(x1, O._net(params, "s", 1, i, weight_sharing))
            t = self.gnn(x1, O._net(params, "t", 1, i, weight_sharing))
            rows = rows + s.sum(dim=1)
            x0 = x0 * torch.exp(s) + t
        return torch.cat([x0, x1], dim=1), rows, c_total

    def per_graph_terms(self, x, params, num_timesteps, weight_sharing=False):
        z, rows, c = self.f_rows(self.to_t(x), self.prep_params(params), num_timesteps, weight_sharing)
        return assemble(z.numpy(), rows.numpy(), c, self.n_node)


def single_graph_batches(n_node, n_edge, senders, receivers, x):
    """the graphs of a batch as batches of their own: (n_node [1], n_edge [1], senders, receivers, x rows), local node ids"""
    n_node = np.asarray(n_node, np.int64)
    n_edge = np.asarray(n_edge, np.int64)
    noff = np.concatenate([[0], np.cumsum(n_node)])
    eoff = np.concatenate([[0], np.cumsum(n_edge)])
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    for g in range(len(n_node)):
        lo, hi = eoff[g], eoff[g + 1]
        yield (n_node[g:g + 1], n_edge[g:g + 1], (s[lo:hi] - noff[g]).astype(np.int32), (r[lo:hi] - noff[g]).astype(np.int32),
               np.asarray(x)[noff[g]:noff[g + 1]])
