"""Float64 reference of the per-graph terms of the sampling direction (gnf_grevnet_inverse_per_graph_f32,
GRevNet.g_per_graph, flow.sample_per_graph).

x = g(z) walks the half-steps backwards; each inverse coupling is x_upd = (z_upd - t) * exp(-s), so its log|det| is
-sum(s), a plain sum over nodes, and each bijector de-normalises with CONSTANTS (the moving statistics): per node its
log|det| is sum_f (0.5 log(moving_var_f + eps) - log gamma_f).  Graph g's share is therefore minus the sum of s over ITS rows
plus n_g times the bijectors' summed term - independent of the other graphs of the batch, with or without batch norm.
`InversePerGraphDense` repeats the loop of the oracle's Fp64Dense.g (same gnn, bn_forward, _net) and keeps -s.sum(axis=1)
per node and each bijector's term; `InversePerGraphGather` does the same on top of the gather formulation of
graph_attn_ref.py (float64 by default, float32 = what fp32 arithmetic costs; the graph scope lives there).  The committed
oracle is not edited."""
import numpy as np

from oracle import gnf_oracle as O

import graph_attn_ref as R
from per_graph_ref import sum_by_graph

LN_2PI = O.LN_2PI


def bn_term(bn):
    """per-node log|det| of bn.forward: sum_f (0.5 log(moving_var_f + eps) - log gamma_f), float64"""
    eps = float(bn.get("epsilon", 1e-3))
    mv = np.asarray(bn["moving_variance"], np.float64)
    gamma = np.asarray(bn["gamma"], np.float64)
    return float(np.sum(0.5 * np.log(mv + eps) - np.log(gamma)))


def assemble(z, x, row_logdet, c_total, n_node):
    """the five [B] vectors flow.sample_per_graph returns (+ x and sumsq), from the INPUT rows z [N, D], the per-node
    log-det of g (= -sum of s) and the bijectors' summed per-node term"""
    z = np.asarray(z, np.float64)
    n_node = np.asarray(n_node, np.int64)
    d = z.shape[1]
    num = n_node.astype(np.float64)
    logdet = sum_by_graph(row_logdet, n_node) + num * c_total
    sumsq = sum_by_graph((z * z).sum(axis=1), n_node)
    zs = -0.5 * sumsq - 0.5 * d * LN_2PI * num
    xs = zs - logdet
    return {"x": np.asarray(x, np.float64), "log_det_jacobian": logdet, "sumsq": sumsq, "log_prob_zs": zs, "log_prob_xs": xs,
            "num_nodes": num, "log_prob_xs_per_node": xs / np.maximum(num, 1.0),
            "row_logdet": np.asarray(row_logdet, np.float64), "c_total": float(c_total)}


class InversePerGraphDense(O.Fp64Dense):
    """Fp64Dense whose g keeps the per-node log-det (same loop, same gnn / bn_forward / _net)."""

    def g_rows(self, z, params, num_timesteps, weight_sharing=False):
        """-> (x [N, D], per-node -sum of s over all half-steps [N], sum over the bijectors of their per-node term)"""
        z = np.asarray(z, np.float64)
        hdim = z.shape[1] // 2
        z0, z1 = z[:, :hdim].copy(), z[:, hdim:].copy()
        rows = np.zeros(z.shape[0], np.float64)
        c_total = 0.0
        bns = params.get("bn")
        for i in reversed(range(num_timesteps)):
            s = self.gnn(z1, O._net(params, "s", 1, i, weight_sharing))
            t = self.gnn(z1, O._net(params, "t", 1, i, weight_sharing))
            rows -= s.sum(axis=1)
            if bns is not None:
                z1 = self.bn_forward(z1, bns[1][i])
                c_total += bn_term(bns[1][i])
            z0 = (z0 - t) * np.exp(-s)
            s = self.gnn(z0, O._net(params, "s", 0, i, weight_sharing))
            t = self.gnn(z0, O._net(params, "t", 0, i, weight_sharing))
            rows -= s.sum(axis=1)
            if bns is not None:
                z0 = self.bn_forward(z0, bns[0][i])
                c_total += bn_term(bns[0][i])
            z1 = (z1 - t) * np.exp(-s)
        return np.concatenate([z0, z1], axis=1), rows, c_total

    def per_graph_terms(self, z, params, num_timesteps, n_node, weight_sharing=False):
        x, rows, c = self.g_rows(z, params, num_timesteps, weight_sharing)
        return assemble(z, x, rows, c, n_node)


class InversePerGraphGather(R.GraphAttnGather):
    """The gather formulation (float64 torch by default; every GNN family, the graph scope included) with the same
    bookkeeping."""

    def g_rows(self, z, params, raw_params, num_timesteps, weight_sharing=False):
        torch = self.torch
        self._mlp_calls = -1
        hdim = z.shape[1] // 2
        z0, z1 = z[:, :hdim], z[:, hdim:]
        rows = torch.zeros(z.shape[0], dtype=self.dtype)
        c_total = 0.0
        bns, raw_bns = params.get("bn"), raw_params.get("bn")
        for i in reversed(range(num_timesteps)):
            s = self.gnn(z1, O._net(params, "s", 1, i, weight_sharing))
            t = self.gnn(z1, O._net(params, "t", 1, i, weight_sharing))
            rows = rows - s.sum(dim=1)
            if bns is not None:
                z1 = self.bn_forward(z1, bns[1][i])
                c_total += bn_term(raw_bns[1][i])
            z0 = (z0 - t) * torch.exp(-s)
            s = self.gnn(z0, O._net(params, "s", 0, i, weight_sharing))
            t = self.gnn(z0, O._net(params, "t", 0, i, weight_sharing))
            rows = rows - s.sum(dim=1)
            if bns is not None:
                z0 = self.bn_forward(z0, bns[0][i])
                c_total += bn_term(raw_bns[0][i])
            z1 = (z1 - t) * torch.exp(-s)
        return torch.cat([z0, z1], dim=1), rows, c_total

    def per_graph_terms(self, z, params, num_timesteps, weight_sharing=False):
        x, rows, c = self.g_rows(self.to_t(z), self.prep_params(params), params, num_timesteps, weight_sharing)
        return assemble(z, x.double().numpy(), rows.double().numpy(), c, self.n_node)
