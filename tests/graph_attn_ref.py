"""Float64 restatement of the whole-graph attention GNNs, MultiheadSelfAttention / SelfAttention (reference gnn.py:576-738),
for the tests of the graph-scope attention (GnfAttn.scope == GNF_ATTN_GRAPH).

`GraphAttnGather` is the oracle's Fp32Gather with attn_gnn taking the graph scope: every node attends to every node of its
own graph, the softmax per graph (the library's form).  `literal_attended` transcribes the reference's own op order - dense
[N, N] logits over the whole batch, loss_mask, `logits -= 100000 * (1 - mask)`, row softmax over the batch - which the CPU
tests pin the restatement against.  `per_graph=True` takes the softmax block by block instead of over dense [heads, N, N]
logits (O(sum n_g^2): large batches); the CPU tests pin it to both.  Parameters: {"attn": {scope: "graph", num_heads, kq_dim, v_dim, kq_dim_division,
layer_norm, wq, wk, wv[, wo][, ln_gamma, ln_beta]}, "mlp": [(W, b), ...]}: no "wo" = SelfAttention."""
import math

import numpy as np

from oracle import gnf_oracle as O


def graph_attn_weight_keys(attn):
    """trainable tensors of one graph-scope block (SelfAttention has no wo)"""
    return ("wq", "wk", "wv") + (("wo",) if "wo" in attn else ()) + \
        (("ln_gamma", "ln_beta") if attn.get("layer_norm", False) else ())


def _keys(attn):
    return graph_attn_weight_keys(attn) if attn.get("scope") == "graph" else O.attn_weight_keys(attn)


class GraphAttnGather(O.Fp32Gather):
    """Fp32Gather (default float64 here) with the graph scope; n_node gives the graphs of the batch."""

    def __init__(self, senders, receivers, n_node, dtype=None, per_graph=False, **kw):
        import torch
        n_node = np.asarray(n_node, np.int64)
        super().__init__(senders, receivers, int(n_node.sum()), dtype=dtype or torch.float64, **kw)
        self.graph_id = torch.as_tensor(np.repeat(np.arange(len(n_node)), n_node))
        self.n_node = n_node
        self.per_graph = per_graph   # True: attended_per_graph, O(sum n_g^2) instead of the dense [heads, N, N]

    def prep_params(self, params):
        def conv(m):
            if isinstance(m, dict) and "gamma" in m:
                return {k: (self.to_t(v) if k != "epsilon" else v) for k, v in m.items()}
            if isinstance(m, dict) and "attn" in m:
                a = dict(m["attn"])
                for key in _keys(a):
                    a[key] = self.to_t(a[key])
                return {"attn": a, "mlp": conv(m["mlp"])}
            if isinstance(m, list) and m and isinstance(m[0], tuple):
                return [(self.to_t(w), self.to_t(b)) for (w, b) in m]
            return [conv(q) for q in m]
        return {k: conv(v) for k, v in params.items()}

    def attended(self, x, a):
        """[N, heads v] attended values, softmax over each node's own graph (columns h v + c)"""
        if self.per_graph:
            return self.attended_per_graph(x, a)
        torch = self.torch
        nh, kq, vd = int(a["num_heads"]), int(a["kq_dim"]), int(a["v_dim"])
        n = x.shape[0]
        q = (x @ a["wq"]).reshape(n, nh, kq)
        k = (x @ a["wk"]).reshape(n, nh, kq)
        v = (x @ a["wv"]).reshape(n, nh, vd)                       # one value projection per head
        logits = torch.einsum("ihd,jhd->hij", q, k)                 # the attending row's q
        if a.get("kq_dim_division", True):
            logits = logits / math.sqrt(kq)
        same = self.graph_id[:, None] == self.graph_id[None, :]
        w = torch.softmax(logits.masked_fill(~same, -float("inf")), dim=-1)
        return torch.einsum("hij,jhc->ihc", w, v).reshape(n, nh * vd)

    def attended_per_graph(self, x, a):
        """attended() block by block: the graphs of one size are stacked into [G, n_g, heads, .] and attend among
        themselves; empty graphs are skipped, a one-node graph's row is its own v (a softmax over one key is 1)."""
        torch = self.torch
        nh, kq, vd = int(a["num_heads"]), int(a["kq_dim"]), int(a["v_dim"])
        n = x.shape[0]
        q = (x @ a["wq"]).reshape(n, nh, kq)
        k = (x @ a["wk"]).reshape(n, nh, kq)
        v = (x @ a["wv"]).reshape(n, nh, vd)
        off = np.concatenate([[0], np.cumsum(self.n_node)])
        rows, parts = [], []
        for size in sorted(set(int(m) for m in self.n_node if m > 0)):
            idx = np.stack([np.arange(off[g], off[g] + size) for g in np.nonzero(self.n_node == size)[0]])   # [G, size]
            it = torch.as_tensor(idx.ravel())
            if size == 1:
                parts.append(v.index_select(0, it))
            else:
                qg = q.index_select(0, it).reshape(len(idx), size, nh, kq)
                kg = k.index_select(0, it).reshape(len(idx), size, nh, kq)
                vg = v.index_select(0, it).reshape(len(idx), size, nh, vd)
                logits = torch.einsum("gihd,gjhd->ghij", qg, kg)
                if a.get("kq_dim_division", True):
                    logits = logits / math.sqrt(kq)
                w = torch.softmax(logits, dim=-1)
                parts.append(torch.einsum("ghij,gjhc->gihc", w, vg).reshape(-1, nh, vd))
            rows.append(idx.ravel())
        if not parts:
            return x.new_zeros((n, nh * vd))
        inv = np.empty(n, np.int64)
        inv[np.concatenate(rows)] = np.arange(n)
        return torch.cat(parts).index_select(0, torch.as_tensor(inv)).reshape(n, nh * vd)

    def attn_gnn(self, x, net):
        a = net["attn"]
        if a.get("scope") != "graph":
            return super().attn_gnn(x, net)
        torch = self.torch
        att = self.attended(x, a)
        new = att @ a["wo"] if "wo" in a else att
        out = self.mlp(torch.cat([x, new], dim=1), net["mlp"])
        if a.get("layer_norm", False):
            mean = out.mean(dim=1, keepdim=True)
            var = ((out - mean) ** 2).mean(dim=1, keepdim=True)
            inv = torch.rsqrt(var + O.LN_EPS) * a["ln_gamma"]
            out = out * inv + (a["ln_beta"] - mean * inv)
        return out


def literal_attended(x, a, n_node):
    """The reference's op order (gnn.py:600-640 / 700-730, loss.py:131-151) in float64 numpy: dense logits over the whole
    batch, the block-diagonal loss_mask, logits -= 100000 (1 - mask), the softmax over the batch row."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    nh, kq, vd = int(a["num_heads"]), int(a["kq_dim"]), int(a["v_dim"])
    q = (x @ np.asarray(a["wq"], np.float64)).reshape(n, nh, kq).transpose(1, 0, 2)
    k = (x @ np.asarray(a["wk"], np.float64)).reshape(n, nh, kq).transpose(1, 0, 2)
    v = (x @ np.asarray(a["wv"], np.float64)).reshape(n, nh, vd).transpose(1, 0, 2)
    logits = q @ k.transpose(0, 2, 1)                               # [heads, N, N]
    if a.get("kq_dim_division", True):
        logits = logits / np.sqrt(float(kq))
    gid = np.repeat(np.arange(len(n_node)), n_node)
    loss_mask = (gid[:, None] == gid[None, :]).astype(np.float64)   # loss.py:131-151
    logits = logits - 100000 * (1 - loss_mask)
    logits = logits - logits.max(axis=-1, keepdims=True)            # (tf.nn.softmax's own max shift)
    e = np.exp(logits)
    w = e / e.sum(axis=-1, keepdims=True)
    att = w @ v                                                     # [heads, N, v]
    return att.transpose(1, 0, 2).reshape(n, nh * vd)


def make_graph_attn_net_params(rng, hdim, latent, num_layers, num_heads=1, kq_dim=10, v_dim=10, out_dim=None,
                               kq_dim_division=True, layer_norm=False, bias_std=0.1, final_scale=1.0, dtype=np.float32):
    """One MultiheadSelfAttention net (out_dim given) or SelfAttention net (out_dim None: one head, no wo): all
    projections xavier-uniform (gnn.py:597-599, 689-691), then the MLP on [x || new]."""
    def xavier(fi, fo):
        lim = math.sqrt(6.0 / (fi + fo))
        return rng.uniform(-lim, lim, size=(fi, fo)).astype(dtype)
    if out_dim is None:
        assert num_heads == 1 and not layer_norm
    attn = {"scope": "graph", "num_heads": num_heads, "kq_dim": kq_dim, "v_dim": v_dim,
            "kq_dim_division": kq_dim_division, "layer_norm": layer_norm,
            "wq": xavier(hdim, num_heads * kq_dim), "wk": xavier(hdim, num_heads * kq_dim),
            "wv": xavier(hdim, num_heads * v_dim)}
    if out_dim is not None:
        attn["wo"] = xavier(num_heads * v_dim, out_dim)
    if layer_norm:
        attn["ln_gamma"] = rng.uniform(0.2, 0.6, hdim).astype(dtype)
        attn["ln_beta"] = (0.1 * rng.standard_normal(hdim)).astype(dtype)
    c = v_dim if out_dim is None else out_dim
    return {"attn": attn, "mlp": O.make_mlp_params(rng, hdim + c, latent, hdim, num_layers, bias_std, final_scale, dtype)}


def make_graph_attn_grevnet_params(seed, hdim, latent, num_layers, num_timesteps, weight_sharing=False, **kw):
    rng = np.random.default_rng(seed)

    def one():
        return make_graph_attn_net_params(rng, hdim, latent, num_layers, **kw)

    if weight_sharing:
        return {"s": [one(), one()], "t": [one(), one()]}
    return {"s": [[one() for _ in range(num_timesteps)] for _ in range(2)],
            "t": [[one() for _ in range(num_timesteps)] for _ in range(2)]}


def hp_of(params, d, latent, k, t, weight_sharing=False, activation="relu"):
    """factories.make_gnn_fn hyper-parameters of a graph-attention parameter set"""
    a = (params["s"][0] if weight_sharing else params["s"][0][0])["attn"]
    attn = {"scope": "graph", "kq_dim": a["kq_dim"], "v_dim": a["v_dim"], "num_heads": a["num_heads"],
            "kq_dim_division": a["kq_dim_division"], "layer_norm": a["layer_norm"]}
    if "wo" in a:
        attn["out_dim"] = int(np.asarray(a["wo"]).shape[1])
    return dict(D=d, latent=latent, K=k, T=t, agg="sum", combine="agg", epsilon=0.0, activation=activation,
                weight_sharing=weight_sharing, attn=attn, use_batch_norm="bn" in params)


def log_prob(n_node, senders, receivers, x, params, num_timesteps, weight_sharing=False, **kw):
    """f + the data term in float64: {"z", "log_det_jacobian", "log_prob_xs", ...} as the oracle's log_prob"""
    o = GraphAttnGather(senders, receivers, n_node, **kw)
    pt = o.prep_params(params)
    z, logdet = o.f(o.to_t(x), pt, num_timesteps, weight_sharing)
    d = z.shape[1]
    lp = (-0.5 * (z * z).sum(dim=1) - 0.5 * d * O.LN_2PI).sum()
    out = O.assemble_log_prob(float(lp), float(logdet), o.n)
    out["z"] = z.numpy()
    return out


def inverse(n_node, senders, receivers, z, params, num_timesteps, weight_sharing=False, **kw):
    o = GraphAttnGather(senders, receivers, n_node, **kw)
    return o.g(o.to_t(z), o.prep_params(params), num_timesteps, weight_sharing).numpy()


def loss_and_grads(n_node, senders, receivers, x, params, num_timesteps, weight_sharing=False, **kw):
    """total_loss = -(sum_n log N(z_n; 0, I) + log_det_jacobian) and its gradient by float64 autograd of the restatement
    (what optimizer.compute_gradients returns, run_grevnet.py:361-362).  grads has the layout of params."""
    o = GraphAttnGather(senders, receivers, n_node, **kw)
    pt = o.prep_params(params)

    def mark(m):
        if isinstance(m, dict) and "attn" in m:
            a = dict(m["attn"])
            for k in _keys(a):
                a[k] = a[k].clone().requires_grad_(True)
            return {"attn": a, "mlp": mark(m["mlp"])}
        if isinstance(m, dict) and "gamma" in m:
            out = dict(m)
            for k in ("gamma", "beta"):
                out[k] = m[k].clone().requires_grad_(True)
            return out
        if isinstance(m, list) and m and isinstance(m[0], tuple):
            return [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for (w, b) in m]
        return [mark(q) for q in m]

    def _grad(w):   # (None: the loss does not reach w - wq, wk of a batch of one-node graphs in the per-graph form)
        return w.grad.numpy().copy() if w.grad is not None else np.zeros(tuple(w.shape), np.float64 if w.dtype == o.torch.float64
                                                                           else np.float32)

    def grads_of(m):
        if isinstance(m, dict) and "attn" in m:
            return {"attn": {k: _grad(m["attn"][k]) for k in _keys(m["attn"])}, "mlp": grads_of(m["mlp"])}
        if isinstance(m, dict) and "gamma" in m:
            return {"gamma": m["gamma"].grad.numpy().copy(), "beta": m["beta"].grad.numpy().copy()}
        if isinstance(m, list) and m and isinstance(m[0], tuple):
            return [(w.grad.numpy().copy(), b.grad.numpy().copy()) for (w, b) in m]
        return [grads_of(q) for q in m]

    pt = {k: mark(v) for k, v in pt.items()}
    z, logdet = o.f(o.to_t(x), pt, num_timesteps, weight_sharing)
    d = z.shape[1]
    log_prob_zs = (-0.5 * (z * z).sum(dim=1) - 0.5 * d * O.LN_2PI).sum()
    total_loss = -(log_prob_zs + logdet)
    total_loss.backward()
    return {"total_loss": float(total_loss.detach()), "log_det_jacobian": float(logdet.detach()), "z": z.detach().numpy(),
            "grads": {k: grads_of(v) for k, v in pt.items()}}


def complete_edges(n_node, self_loops=True):
    """senders, receivers of the complete graphs (with self loops) of a batch, global node ids"""
    s, r, off = [], [], 0
    for nn in n_node:
        ii, jj = np.meshgrid(np.arange(nn), np.arange(nn), indexing="ij")
        keep = np.ones_like(ii, bool) if self_loops else ii != jj
        s.append(ii[keep].ravel() + off)
        r.append(jj[keep].ravel() + off)
        off += nn
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return cat(s), cat(r)
