"""Training step of the GRevNet drivers (/root/reference/run_grevnet.py:340-377, 440-447; same at
train_grevnet_with_data.py:356-395) on the MI355X kernels:

    grads_and_vars = optimizer.compute_gradients(total_loss)      -> gnf_grevnet_backward_f32 (reversible backprop)
    tf.clip_by_value / tf.clip_by_norm on every gradient           -> gnf_clip_by_value_f32 / gnf_clip_by_norm_f32
    tf.train.AdamOptimizer(lr, beta1, beta2, epsilon).apply_gradients -> gnf_adam_f32 + gnf_pack_flow

Every trainable variable of the flow lives in ONE flat fp32 device vector (`theta`; the MLPs' W / b are
views into it, in snt.Linear's own [in, out] layout), the gradient, and Adam's two moment vectors have
the same layout: the optimiser is one elementwise launch over the whole model, and the data-parallel
gradient exchange is one flat all-reduce (RCCL over xGMI), not one collective per variable.

The drivers' default learning-rate decay (tf.train.exponential_decay, run_grevnet.py:341-347) is one line of
`current_learning_rate`; any other schedule is the caller's business (`step(graph, learning_rate=...)`; the
--use_lr_schedule function lives in examples/driver_utils.py: out of this path's scope).

The trainer's state (what tf.train.Saver checkpoints for the drivers, run_grevnet.py:379,449-453: variables, Adam slots,
global_step, the bijectors' moving statistics) is `trainer_state` / `load_trainer_state` / `save_checkpoint` /
`load_checkpoint` below; bench.py restores it before every timed region of a training workload.
"""
import ctypes as C
import math

import torch

from . import _abi
from .gnn import _EPOCH, _touch as _gnn_touch
from .flow import LN_2PI
from .graphs import csr_desc, csr_of
from .params import ParamArena


def _adopt(trainer, arena):
    """the trainer's public theta / grad / m / v are the arena's"""
    trainer.theta, trainer.grad, trainer.m, trainer.v = arena.theta, arena.grad, arena.m, arena.v


def _host_copy(tree):
    """a container of device tensors as the same container of numpy arrays"""
    if isinstance(tree, dict):
        return {k: _host_copy(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_host_copy(v) for v in tree)
    return tree.detach().cpu().numpy().copy()


def _adam_step(tr, learning_rate, stream):
    """tf.train.AdamOptimizer(lr, beta1, beta2, epsilon).apply_gradients over the whole arena: the bias-corrected step size
    of step global_step + 1 on the host, one gnf_adam_f32 launch (the caller has made theta's device current)."""
    t = tr.global_step + 1
    lr_t = learning_rate * math.sqrt(1.0 - tr.beta2 ** t) / (1.0 - tr.beta1 ** t)
    _abi.check(_abi.lib().gnf_adam_f32(_abi.ptr(tr.theta), _abi.ptr(tr.grad), _abi.ptr(tr.m), _abi.ptr(tr.v), tr.theta.numel(),
                                       lr_t, tr.beta1, tr.beta2, tr.epsilon, stream), "gnf_adam_f32")
    tr.global_step = t


class _StepTerms(dict):
    """values_map of a training iteration (run_grevnet.py:290-302).  The two batch sums come out of the flow as device
    fp64 scalars; every derived scalar (log_prob_zs, total_loss, the *_per_node values ...) is a few 0-d torch
    operations that are only launched when somebody asks for the value (a training loop that logs every n-th step
    pays for them every n-th step, not ~10 small launches per iteration)."""
    _DERIVED = ("log_det_jacobian", "log_prob_zs", "log_prob_xs", "total_loss", "loss_per_node", "log_prob_xs_per_node",
                "log_prob_zs_per_node", "log_det_jacobian_per_node")

    def __init__(self, z_graph, reconstruction, sums, n, d):
        super().__init__(z_graph=z_graph, reconstruction=reconstruction, num_nodes=float(n), sums=sums)
        self._n, self._d = float(n), int(d)

    def __missing__(self, key):
        if key not in self._DERIVED:
            raise KeyError(key)
        sums, n = dict.__getitem__(self, "sums"), self._n
        logdet = sums[0]
        log_prob_zs = -0.5 * sums[1] - 0.5 * self._d * LN_2PI * n
        log_prob_xs = log_prob_zs + logdet
        vals = {"log_det_jacobian": logdet, "log_prob_zs": log_prob_zs, "log_prob_xs": log_prob_xs,
                "total_loss": -log_prob_xs, "loss_per_node": -log_prob_xs / n, "log_prob_xs_per_node": log_prob_xs / n,
                "log_prob_zs_per_node": log_prob_zs / n, "log_det_jacobian_per_node": logdet / n}
        return vals[key]   # not cached: `sums` may be rewritten in place (captured-graph replay)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._DERIVED

    def get(self, key, default=None):
        return self[key] if key in self else default


class GRevNetTrainer:
    """total_loss, its gradient and the Adam update for one GRevNet (message-passing GNNs with or without the
    batch-norm bijectors, and the edge-list attention GNN: every variable the reference's optimizer would see).

    Hyper-parameters default to the drivers' flags (run_grevnet.py:114-131): lr 1e-4, beta1 0.9,
    beta2 0.9, epsilon 1e-8, exponential lr decay (1000 steps, 0.96), no clipping."""

    def __init__(self, grevnet, lr=1e-4, adam_beta1=0.9, adam_beta2=0.9, adam_epsilon=1e-8, use_lr_decay=True,
                 lr_decay_steps=1000, lr_decay_rate=0.96, clip_gradient_by_value=False,
                 clip_gradient_value_lower=-1.0, clip_gradient_value_upper=5.0, clip_gradient_by_norm=False,
                 clip_gradient_norm=10.0):
        self.net = grevnet
        self.lr, self.beta1, self.beta2, self.epsilon = float(lr), float(adam_beta1), float(adam_beta2), float(adam_epsilon)
        self.use_lr_decay, self.lr_decay_steps, self.lr_decay_rate = bool(use_lr_decay), int(lr_decay_steps), float(lr_decay_rate)
        self.clip_by_value = bool(clip_gradient_by_value)
        self.clip_lo, self.clip_hi = float(clip_gradient_value_lower), float(clip_gradient_value_upper)
        self.clip_by_norm, self.clip_norm = bool(clip_gradient_by_norm), float(clip_gradient_norm)
        self.global_step = 0
        self.theta = self.grad = self.m = self.v = None
        self._arena = ParamArena()
        self._grads = None       # views of self.grad in get_params()'s layout (named_gradients)
        self._grad_flow = None
        self._keep = None
        self._offsets = None
        self._ws = None
        self._bns = []
        self._clip_ws = None     # scratch of the two-pass clip_by_norm
        self._stash = None       # attention front-end stash (uint8 device buffer), see loss_and_grads
        self.stash_attention = True          # False: recompute the attention front-end in the backward walk
        self.stash_mlp_rows = True           # False: recompute the MLP rows too (the fully reversible walk)
        self._mlp_stash = None
        self._aux = None         # second HIP stream: the weight-gradient GEMMs overlap the backward walk
        self.overlap_weight_grads = True     # False: no auxiliary stream for the weight-gradient GEMMs
        # the MLP-row stash is memory for time (wide nets: 2T slots of every hidden activation - about 20 GB for 30 k nodes
        # at the data driver's defaults): it is taken only while it fits this budget; beyond it the walk recomputes.
        # None = at most `mlp_stash_free_fraction` of the memory the device has free when the stash is first needed.
        self.mlp_stash_max_bytes = None
        self.mlp_stash_free_fraction = 0.5
        self.mlp_stash_declined = None       # (bytes asked, reason) of the last stash that was NOT taken

    # ---- parameter arena ---------------------------------------------------------------------
    def _ensure_arena(self, hdim, device):
        """theta / grad / m / v over every variable of the flow, in ONE order: the MLPs of s then t ((W, b) per layer), the
        attention blocks of s then t (attn_keys()), the bijectors' gamma, beta (index half*T + i; their moving statistics are
        not trained).  Re-seated when somebody called set_params / set_attn_params (or moved the net) since: their tensors
        live OUTSIDE theta, so Adam would go on updating a vector nothing reads."""
        net, arena = self.net, self._arena
        net._flow(hdim, device)                      # builds lazily-initialised MLPs (Sonnet-style first connect)
        if arena.is_seated(device, _EPOCH[0]):
            return
        mlps = net.mlps("s") + net.mlps("t")
        blocks = [b for b in net.blocks("s") + net.blocks("t") if getattr(b, "attn_params", None) is not None]
        bns = [b for half in net.bns for b in half] if net.use_batch_norm else []
        slots = [(m, "params", j, h) for m in mlps for j in range(len(m.params)) for h in (0, 1)]
        slots += [(b, "attn_params", k) for b in blocks for k in b.attn_keys()]
        slots += [(b, k) for b in bns for k in ("gamma", "beta")]
        _adopt(self, arena.seat(slots, device))
        for c in mlps + bns:                          # the containers now read / are updated through the arena
            c.version += 1
            _gnn_touch()
        for b in blocks:
            b._attn_version += 1
            _gnn_touch()
        net._cache = None
        arena.epoch = _EPOCH[0]
        self._offsets, self._bns = arena.offsets, bns
        # the gradient in the parameter container's layout (named_gradients) and as a flow descriptor: same shapes, every
        # pointer a view of self.grad
        g = iter(arena.grad_views)
        g_mlps = [[(next(g), next(g)) for _ in m.params] for m in mlps]
        g_attn = [{k: next(g) for k in b.attn_keys()} for b in blocks]
        g_bns = [{"gamma": next(g), "beta": next(g)} for _ in bns]
        n, t = len(mlps) // 2, net.num_timesteps
        nets = [{"attn": a, "mlp": m} for a, m in zip(g_attn, g_mlps)] if blocks else g_mlps
        halves = lambda flat: flat if net.weight_sharing else [flat[:t], flat[t:]]
        self._grads = {"s": halves(nets[:n]), "t": halves(nets[n:])}
        if bns:
            self._grads["bn"] = [g_bns[:t], g_bns[t:]]
        gs, gt = (_abi.GnfMlp * n)(), (_abi.GnfMlp * n)()
        for q, (m, layers) in enumerate(zip(mlps, g_mlps)):
            desc = (gs if q < n else gt)[q % n]
            desc.num_layers = len(m.layer_sizes)
            for j, d in enumerate(m.dims()):
                desc.dims[j] = d
            for j, (gw, gb) in enumerate(layers):
                desc.W[j], desc.b[j] = gw.data_ptr(), gb.data_ptr()
        gattn = (_abi.GnfAttn * len(blocks))() if blocks else None   # gradient GnfAttn per net, hung off the gradient GnfMlp
        for q, (blk, ptrs) in enumerate(zip(blocks, g_attn)):       # order: s nets then t nets
            ga = gattn[q]
            ga.num_heads, ga.kq_dim, ga.v_dim, ga.out_dim = blk.num_heads, blk.kq_dim, blk.v_dim, blk.concat_heads_output_dim
            ga.layer_norm = int(blk.layer_norm)
            ga.scope = _abi.GNF_ATTN_GRAPH if blk.graph_scope else _abi.GNF_ATTN_EDGES
            ga.Wq, ga.Wk, ga.Wv = ptrs["wq"].data_ptr(), ptrs["wk"].data_ptr(), ptrs["wv"].data_ptr()
            ga.Wo = ptrs["wo"].data_ptr() if "wo" in ptrs else 0      # (SelfAttention: no wo)
            if blk.layer_norm:
                ga.ln_gamma, ga.ln_beta = ptrs["ln_gamma"].data_ptr(), ptrs["ln_beta"].data_ptr()
            (gs if q < n else gt)[q % n].attn = C.cast(C.byref(gattn, q * C.sizeof(_abi.GnfAttn)), C.POINTER(_abi.GnfAttn))
        gbn = (_abi.GnfBatchNorm * len(bns))() if bns else None
        for q, gd in enumerate(g_bns):
            gbn[q].gamma, gbn[q].beta = gd["gamma"].data_ptr(), gd["beta"].data_ptr()
        self._grad_flow = _abi.GnfFlow(net.num_timesteps, int(net.weight_sharing),
                                       C.cast(gs, C.POINTER(_abi.GnfMlp)), C.cast(gt, C.POINTER(_abi.GnfMlp)),
                                       net.blocks("s")[0].spec(),
                                       C.cast(gbn, C.POINTER(_abi.GnfBatchNorm)) if gbn is not None else None)
        self._keep = (gs, gt, gbn, gattn)

    def named_gradients(self):
        """Gradients in the oracle / fixture container layout ({"s": [[mlp]*T, [mlp]*T], "t": ...}; mlp = [(dW, db), ...],
        attention nets {"attn": {...}, "mlp": mlp}; "bn": [[{gamma, beta}]*T]*2) as numpy arrays (host copy; for tests and
        summaries)."""
        return _host_copy(self._grads)

    # ---- compute_gradients ---------------------------------------------------------------------
    def loss_and_grads(self, graph):
        """run_grevnet.py:291-302 + optimizer.compute_gradients(total_loss) (:361-362).  Leaves the gradient in
        self.grad (flat, arena layout) and returns the scalar terms (0-d fp64 device tensors)."""
        lib = _abi.lib()
        net = self.net
        x = graph.nodes
        if x.device.type != "cuda":
            raise _abi.GnfError("training runs on a HIP device only (no CPU path)")
        n, d = x.shape
        dev = x.device
        self._ensure_arena(d // 2, dev)
        # attention GNNs: the forward pass leaves every half-step's front-end (q | k | v, layer-0 inputs) in a stash
        # the backward pass reads instead of recomputing it (memory for time: 2T slots; stash_attention=False keeps
        # the fully reversible, recompute-everything walk)
        fwd_flow = net._flow(d // 2, dev)
        with torch.cuda.device(dev):   # (the planners behind these sizes read the CURRENT device's CU count)
            stash_bytes = lib.gnf_attn_stash_bytes(n, d, C.byref(fwd_flow)) if self.stash_attention else 0
            mlp_bytes = lib.gnf_mlp_stash_bytes(n, d, C.byref(fwd_flow)) if self.stash_mlp_rows else 0
        if stash_bytes:
            if self._stash is None or self._stash.numel() < stash_bytes or self._stash.device != dev:
                self._stash = torch.empty(stash_bytes, dtype=torch.uint8, device=dev)
            fwd_flow.attn_stash, fwd_flow.attn_stash_bytes = self._stash.data_ptr(), stash_bytes
        # message-passing nets on small batches: the same trade for the MLP rows (layer-0 inputs, hidden activations,
        # s and t of every half-step - what TensorFlow keeps for tf.gradients anyway): the backward kernels skip their
        # recompute half.  gnf_mlp_stash_bytes is 0 where the library would not use a stash.
        if mlp_bytes and not self._ensure_mlp_stash(mlp_bytes, dev):
            mlp_bytes = 0          # (GnfFlow.mlp_stash = NULL: the backward walk recomputes the MLP rows)
        if mlp_bytes:
            fwd_flow.mlp_stash, fwd_flow.mlp_stash_bytes = self._mlp_stash.data_ptr(), mlp_bytes
        try:
            return self._loss_and_grads(graph, n, d, dev)
        finally:   # plain forward calls of the same net must not write into (or rely on) the stashes
            fwd_flow.attn_stash, fwd_flow.attn_stash_bytes = None, 0
            fwd_flow.mlp_stash, fwd_flow.mlp_stash_bytes = None, 0

    def _ensure_mlp_stash(self, mlp_bytes, dev):
        """Make self._mlp_stash hold `mlp_bytes` on `dev` if the budget allows; False = train without the stash."""
        if self._mlp_stash is not None and self._mlp_stash.numel() >= mlp_bytes and self._mlp_stash.device == dev:
            return True
        self._mlp_stash = None     # (a smaller one is released before the larger one is asked for)
        free, _total = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)   # the caching allocator's idle blocks
        ok, why = mlp_stash_within_budget(mlp_bytes, free, self.mlp_stash_max_bytes, self.mlp_stash_free_fraction)
        if ok:
            try:
                self._mlp_stash = torch.empty(mlp_bytes, dtype=torch.uint8, device=dev)
                self.mlp_stash_declined = None
                return True
            except torch.OutOfMemoryError:
                why = "allocation failed (device out of memory)"
        self.mlp_stash_declined = (int(mlp_bytes), why)
        return False

    def _loss_and_grads(self, graph, n, d, dev):
        lib = _abi.lib()
        net = self.net
        z, sums = net._run(graph, _abi.GNF_FORWARD)               # f: fused forward kernels
        net.last_sums = sums
        z_graph = graph.replace(nodes=z)
        flow = net._flow(d // 2, dev)
        csr, csr_t = csr_desc(graph, csr_of(graph), net.graph_scope()), csr_of(graph, by_sender=True)
        ws_bytes = lib.gnf_backward_workspace_bytes(n, d, C.byref(flow))
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != dev:
            self._ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        if self.overlap_weight_grads and (self._aux is None or self._aux.device != dev):
            self._aux = torch.cuda.Stream(device=dev)
        if not self.overlap_weight_grads:
            self._aux = None
        state = z_graph.nodes.clone()                             # z in, x (reconstructed) out
        with torch.cuda.device(dev):
            _abi.check(lib.gnf_grevnet_backward_f32(C.byref(csr), C.byref(csr_t.desc), C.byref(flow),
                                                    C.byref(self._grad_flow), _abi.ptr(state), state.stride(0), d,
                                                    _abi.ptr(self._ws), ws_bytes, _abi.stream_ptr(dev),
                                                    C.c_void_p(self._aux.cuda_stream if self._aux is not None else 0)),
                       "gnf_grevnet_backward_f32")
        return _StepTerms(z_graph, state, sums, n, d)

    # ---- apply_gradients -----------------------------------------------------------------------
    def current_learning_rate(self):
        if self.use_lr_decay:   # tf.train.exponential_decay(lr, global_step, decay_steps, decay_rate), run_grevnet.py:341-347
            return self.lr * self.lr_decay_rate ** (self.global_step / float(self.lr_decay_steps))
        return self.lr

    def apply_gradients(self, learning_rate=None):
        """Clipping (run_grevnet.py:363-373) then tf.train.AdamOptimizer.apply_gradients (:375) and the re-pack
        of the matrix-core weight copies."""
        lib = _abi.lib()
        dev = self.theta.device
        lr = self.current_learning_rate() if learning_rate is None else float(learning_rate)
        n = self.theta.numel()
        with torch.cuda.device(dev):
            st = _abi.stream_ptr(dev)
            if self.clip_by_value:
                _abi.check(lib.gnf_clip_by_value_f32(_abi.ptr(self.grad), n, self.clip_lo, self.clip_hi, st),
                           "gnf_clip_by_value_f32")
            if self.clip_by_norm:
                nt = self._offsets.numel() - 1
                cb = lib.gnf_clip_workspace_bytes(nt)
                if self._clip_ws is None or self._clip_ws.numel() < cb or self._clip_ws.device != dev:
                    self._clip_ws = torch.empty(max(cb, 8), dtype=torch.uint8, device=dev)
                _abi.check(lib.gnf_clip_by_norm_f32(_abi.ptr(self.grad), _abi.ptr(self._offsets), nt, self.clip_norm,
                                                    _abi.ptr(self._clip_ws), cb, st), "gnf_clip_by_norm_f32")
            _adam_step(self, lr, st)
            h = self.net.mlps("s")[0].layer_sizes[-1]
            flow = self.net._flow(h, dev)
            if self.net.fused:
                _abi.check(lib.gnf_pack_flow(C.byref(flow), st), "gnf_pack_flow")
            if self._bns:          # gamma_constraint projection (gnn.py:261-262) + UPDATE_OPS (run_grevnet.py:360), one launch
                _abi.check(lib.gnf_bn_post_step_f32(C.byref(flow), h, self._bns[0].momentum, st), "gnf_bn_post_step_f32")

    def all_reduce_gradients(self, group=None):
        """Data parallelism: total_loss is a SUM over nodes (run_grevnet.py:295), so the gradient of the global
        batch is the sum of the shard gradients: one flat all-reduce of the whole gradient vector."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            if self.grad.is_cuda and dist.get_backend(group) == "gloo":
                host = self.grad.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
                self.grad.copy_(host)
            else:
                dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)

    def step(self, graph, learning_rate=None, all_reduce=False):
        """One iteration of the training loop (run_grevnet.py:440-447): returns the scalars of values_map."""
        out = self.loss_and_grads(graph)
        if all_reduce:
            self.all_reduce_gradients()
        self.apply_gradients(learning_rate)
        return out


def mlp_stash_within_budget(stash_bytes, free_bytes, max_bytes=None, free_fraction=0.5):
    """The trainer's rule for taking the MLP-row stash (pure arithmetic: tests/test_host_logic_cpu.py): within the caller's
    cap when there is one, else within `free_fraction` of the device memory currently free (the backward workspace, the
    attention stash and the next batch have to fit beside it).  Returns (ok, reason)."""
    if max_bytes is not None:
        if stash_bytes > max_bytes:
            return False, f"{stash_bytes} bytes > mlp_stash_max_bytes = {max_bytes}"
        return True, ""
    if stash_bytes > free_fraction * free_bytes:
        return False, f"{stash_bytes} bytes > {free_fraction:g} x {free_bytes} bytes free on the device"
    return True, ""


# ---- the trainer's state: what the drivers checkpoint through tf.train.Saver (run_grevnet.py:379, 449-453) --------------
def _state(tr, bns):
    if tr.theta is None:
        raise RuntimeError("run a step (or loss_and_grads) first so that the variables exist")
    return {"theta": tr.theta.detach().cpu(), "m": tr.m.detach().cpu(), "v": tr.v.detach().cpu(),
            "global_step": tr.global_step,
            "bn_moving": [(b.moving_mean.detach().cpu(), b.moving_variance.detach().cpu()) for b in bns]}


def _load_state(tr, bns, state, what):
    if tr.theta is None:
        raise RuntimeError("connect the trainer first (run loss_and_grads on a batch)")
    if state["theta"].numel() != tr.theta.numel():
        raise ValueError(f"checkpoint has {state['theta'].numel()} parameters, the {what} has {tr.theta.numel()}")
    tr.theta.copy_(state["theta"])
    tr.m.copy_(state["m"])
    tr.v.copy_(state["v"])
    tr.global_step = int(state["global_step"])
    for b, (mm, mv) in zip(bns, state["bn_moving"]):
        b.moving_mean.copy_(mm)
        b.moving_variance.copy_(mv)


def trainer_state(tr):
    """Everything a resumed run needs: parameters, Adam moments, step counter, batch-norm moving statistics (host copies)."""
    return _state(tr, tr._bns)


def load_trainer_state(tr, state):
    """Restore `trainer_state`'s dict into a connected trainer; the matrix-core weight copies follow (gnf_pack_flow)."""
    _load_state(tr, tr._bns, state, "flow")
    dev = tr.theta.device
    with torch.cuda.device(dev):
        flow = tr.net._flow(tr.net.mlps("s")[0].layer_sizes[-1], dev)
        if tr.net.fused:
            _abi.check(_abi.lib().gnf_pack_flow(C.byref(flow), _abi.stream_ptr(dev)), "gnf_pack_flow")


def save_checkpoint(tr, path):
    torch.save(trainer_state(tr), path)


def load_checkpoint(tr, path):
    load_trainer_state(tr, torch.load(path, map_location="cpu"))


# ==== stage 1: the graph auto-encoder's training step (run_gnn.py:230-296) ======================================================
class EncoderTrainer:
    """total_loss = binary_loss' sum_loss (run_gnn.py:255-270; the reference's regularisers are commented out, gnn.py:175-178),
    its gradient through gnn.TimestepGNN and the Adam update, for the message-passing GNNs:

        gnn(graph, is_training=True)                  -> gnf_timestep_gnn_train_forward_f32 (the moving statistics advance here,
                                                         once per step: what the UPDATE_OPS dependency does, run_gnn.py:295)
        binary_loss(gnn_output, true_graph, ...)      -> gnf_adj_loss_f32 with grad="sum"
        optimizer.minimize(total_loss)                -> gnf_timestep_gnn_backward_f32 + gnf_adam_f32

    Every trainable variable (the nets' W / b, the batch norms' and layer norms' gamma / beta) lives in ONE flat fp32 device
    vector `theta`, the gradient and Adam's two moment vectors share its layout, so the optimiser is one launch.  The defaults
    are run_gnn.py's flags (lr 1e-4, beta1 0.9, beta2 0.999, epsilon 1e-8, lr_type polynomial_decay over num_train_iters
    200000); lr_type "schedule" is not built.  No clipping: run_gnn.py has none.  With max_nodes_per_graph given,
    loss_and_grads neither copies to the host nor synchronises and can be captured; apply_gradients is one more launch whose
    step size is a host scalar that changes every step (it is passed by value, so it stays outside a captured region).
    tune_sigmoid (run_gnn.py:146-165): temp and shift of sigmoid_l2 are trained as well.  distance_fn is then a sigmoid_l2 or
    adj_loss.TunedSigmoidL2 token (its values are where training starts); the two floats are the LAST two entries of theta,
    self.distance_fn is a TunedSigmoidL2 whose .params is a view of them, binary_loss writes their gradient into the last two
    entries of grad (gnf_adj_loss_dist_f32) and the one Adam launch moves them with everything else.  The kernels read them
    from the device at run time, so a captured loss_and_grads replayed after a step computes what the eager call computes.
    loss_type "triplet" (run_gnn.py:249-252) puts triplet_loss.triplet_loss in binary_loss' place: total_loss is the sum of the
    node losses (run_gnn.py:270 adds a sum_loss its triplet branch never defines), the scores are triplet_dist_fn's (l2), the
    terms triplet_loss_fn's (margin_loss()), the edge-error counts come from one binary_loss call without a gradient under
    triplet_adj_dist_fn (hacky_sigmoid_l2).  The samples of a step are those of seed + global_step, a host scalar: a captured
    loss_and_grads replays the same samples; for fresh ones under capture pass `draws` (uint32 [L, 2, N] on the device) and
    refill it between replays.  tune_sigmoid with "triplet" is a ValueError."""

    LR_TYPES = ("constant", "fixed_decay", "polynomial_decay")
    LOSS_TYPES = ("binary", "triplet")

    def __init__(self, encoder, lr=1e-4, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, lr_type="polynomial_decay",
                 num_train_iters=200000, lr_fixed_decay_steps=1000, lr_fixed_decay_rate=0.99, lr_fixed_decay_staircase=False,
                 distance_fn=None, use_soft_labels=False, max_nodes_per_graph=None, tune_sigmoid=False, loss_type="binary",
                 triplet_dist_fn=None, triplet_adj_dist_fn=None, triplet_loss_fn=None, num_sampling_loops=8, seed=0, draws=None):
        from .adj_loss import TunedSigmoidL2, check_token, hacky_sigmoid_l2, sigmoid_l2
        from .flow import scaled_hacky_sigmoid_l2
        from .triplet_loss import MAX_SAMPLING_LOOPS, l2, loss_params, margin_loss, score_params
        if lr_type not in self.LR_TYPES:
            raise ValueError(f"lr_type={lr_type!r}: one of {self.LR_TYPES} ('schedule' is not built)")
        if loss_type not in self.LOSS_TYPES:
            raise ValueError(f"loss_type={loss_type!r}: one of {self.LOSS_TYPES}")
        self.loss_type = loss_type
        self.tune_sigmoid = bool(tune_sigmoid)
        if loss_type == "triplet":
            if self.tune_sigmoid:
                raise ValueError("tune_sigmoid trains the parameters of binary_loss' distance function: no parameter gradient is "
                                 "built under loss_type='triplet'")
            self.triplet_dist_fn = l2 if triplet_dist_fn is None else triplet_dist_fn
            self.triplet_loss_fn = margin_loss() if triplet_loss_fn is None else triplet_loss_fn
            self.triplet_adj_dist_fn = hacky_sigmoid_l2 if triplet_adj_dist_fn is None else triplet_adj_dist_fn
            score_params(self.triplet_dist_fn), loss_params(self.triplet_loss_fn)   # NotImplementedError now, not at step 1
            if isinstance(self.triplet_adj_dist_fn, TunedSigmoidL2):
                raise NotImplementedError("triplet_adj_dist_fn: one of the three sigmoid tokens with constant parameters")
            check_token(self.triplet_adj_dist_fn, "triplet_adj_dist_fn")
            if not 1 <= int(num_sampling_loops) <= MAX_SAMPLING_LOOPS:
                raise ValueError(f"num_sampling_loops={num_sampling_loops}: 1 to {MAX_SAMPLING_LOOPS}")
        self.num_sampling_loops, self.seed, self.draws = int(num_sampling_loops), int(seed), draws
        if self.tune_sigmoid:
            if isinstance(distance_fn, sigmoid_l2):
                distance_fn = TunedSigmoidL2(distance_fn.temp, distance_fn.shift)
            elif not isinstance(distance_fn, TunedSigmoidL2):   # run_gnn.py:148-153
                raise ValueError("tune_sigmoid needs distance_fn = sigmoid_l2(temp, shift) or TunedSigmoidL2(temp, shift)")
        self.net = encoder
        self.lr, self.beta1, self.beta2, self.epsilon = float(lr), float(adam_beta1), float(adam_beta2), float(adam_epsilon)
        self.lr_type, self.num_train_iters = lr_type, int(num_train_iters)
        self.lr_fixed_decay_steps, self.lr_fixed_decay_rate = int(lr_fixed_decay_steps), float(lr_fixed_decay_rate)
        self.lr_fixed_decay_staircase = bool(lr_fixed_decay_staircase)
        self.distance_fn = scaled_hacky_sigmoid_l2 if distance_fn is None else distance_fn
        self.use_soft_labels = bool(use_soft_labels)
        self.max_nodes_per_graph = max_nodes_per_graph
        self.global_step = 0
        self.theta = self.grad = self.m = self.v = None
        self._arena = ParamArena()
        self._grads = None     # views of self.grad in TimestepGNN.make_grads' layout

    # ---- parameter arena ---------------------------------------------------------------------
    def _ensure_arena(self, d, device):
        """theta / grad / m / v in ONE order: the nets' (W, b) per layer, the batch norms' gamma, beta per timestep, the
        layer norms', then (tune_sigmoid) temp, shift.  Re-seated when somebody called set_params (or moved the encoder)."""
        net, arena = self.net, self._arena
        if arena.is_seated(device, _EPOCH[0]):
            return
        net._desc(d, torch.device(device), True)  # creates the variables at first connection (Sonnet style)
        mlps, norms = [b._mlp for b in net.blocks()], list(net.bns) + list(net.lns)
        slots = [(m, "params", j, h) for m in mlps for j in range(len(m.params)) for h in (0, 1)]
        slots += [(o, k) for o in norms for k in ("gamma", "beta")]
        if self.tune_sigmoid:                     # temp, shift: the last two entries
            sigmoid = self.distance_fn.values()   # (a host read, when the arena is laid out only)
        _adopt(self, arena.seat(slots, device, trailing=2 if self.tune_sigmoid else 0))
        for c in mlps + norms:                    # the containers now read / are updated through the arena
            c.version += 1
            _gnn_touch()
        arena.epoch = _EPOCH[0]
        g = iter(arena.grad_views)
        self._grads = {"nets": [[(next(g), next(g)) for _ in m.params] for m in mlps]}
        for key, objs in (("bn", net.bns), ("ln", net.lns)):
            if objs:
                self._grads[key] = [{"gamma": next(g), "beta": next(g)} for _ in objs]
        if self.tune_sigmoid:
            arena.tail.copy_(torch.tensor(sigmoid, dtype=torch.float32))
            self.distance_fn.bind(arena.tail)

    def named_gradients(self):
        """The gradients in TimestepGNN.get_params()'s layout (without the moving statistics) as numpy arrays (host copy)."""
        return _host_copy(self._grads)

    # ---- compute_gradients -----------------------------------------------------------------------
    def loss_and_grads(self, graph, true_graph=None):
        """Train-forward, binary_loss against true_graph (default: the batch itself; another one is the denoising case of
        run_gnn.py:238) and the backward pass.  Leaves the gradient of total_loss = sum_loss in self.grad and returns
        binary_loss' result dict plus "gnn_output" and "total_loss" (device tensors, nothing read back)."""
        from . import adj_loss
        x = graph.nodes
        if x.device.type != "cuda":
            raise _abi.GnfError("training runs on a HIP device only (no CPU path)")
        self._ensure_arena(int(x.shape[1]), x.device)
        out, stash = self.net.forward_train(graph)
        if self.loss_type == "triplet":
            return self._triplet_loss_and_grads(graph, graph if true_graph is None else true_graph, out, stash)
        res = adj_loss.binary_loss(out, graph if true_graph is None else true_graph, distance_fn=self.distance_fn,
                                   use_soft_labels=self.use_soft_labels, grad="sum",
                                   max_nodes_per_graph=self.max_nodes_per_graph,
                                   grad_params=self.grad[-2:] if self.tune_sigmoid else False)
        self.net.backward(graph, stash, res["grad_nodes"], self._grads)
        res["gnn_output"], res["total_loss"] = out, res["sum_loss"]
        return res

    def _triplet_loss_and_grads(self, graph, true_graph, out, stash):
        """loss_type "triplet" behind the training forward: triplet_loss with grad="sum" on the samples of seed + global_step (or
        of self.draws), one binary_loss call without a gradient under triplet_adj_dist_fn for the edge-error counts, backward.
        The result holds triplet_loss' keys ("sum_loss" and "mean_loss" are the triplet loss'), the two count tensors of
        binary_loss, "gnn_output" and "total_loss" = the summed node losses."""
        from . import adj_loss
        from .triplet_loss import triplet_loss
        res = triplet_loss(out, true_graph, distance_fn=self.triplet_dist_fn, triplet_loss_fn=self.triplet_loss_fn,
                              num_sampling_loops=self.num_sampling_loops, seed=self.seed + self.global_step, draws=self.draws,
                              grad="sum", max_nodes_per_graph=self.max_nodes_per_graph)
        counts = adj_loss.binary_loss(out, true_graph, distance_fn=self.triplet_adj_dist_fn, grad=None,
                                      max_nodes_per_graph=self.max_nodes_per_graph)
        self.net.backward(graph, stash, res["grad_nodes"], self._grads)
        res["false_positive_pairs"], res["false_negative_pairs"] = counts["false_positive_pairs"], counts["false_negative_pairs"]
        res["gnn_output"], res["total_loss"] = out, res["sum_loss"]
        return res

    # ---- apply_gradients -------------------------------------------------------------------------
    def current_learning_rate(self):
        """run_gnn.py:275-288 on the host: constant | tf.train.exponential_decay | tf.train.polynomial_decay(decay_steps =
        num_train_iters, end_learning_rate = lr / 100, power = 0.5)"""
        return encoder_learning_rate(self.lr_type, self.lr, self.global_step, self.num_train_iters, self.lr_fixed_decay_steps,
                                     self.lr_fixed_decay_rate, self.lr_fixed_decay_staircase)

    def apply_gradients(self, learning_rate=None):
        """tf.train.AdamOptimizer(lr, beta1, beta2, epsilon).apply_gradients: one gnf_adam_f32 over the arena"""
        dev = self.theta.device
        lr = self.current_learning_rate() if learning_rate is None else float(learning_rate)
        with torch.cuda.device(dev):
            _adam_step(self, lr, _abi.stream_ptr(dev))

    def step(self, graph, true_graph=None, learning_rate=None):
        """One iteration of run_gnn.py's loop: returns loss_and_grads' dict."""
        out = self.loss_and_grads(graph, true_graph)
        self.apply_gradients(learning_rate)
        return out


def encoder_learning_rate(lr_type, lr, global_step, num_train_iters=200000, decay_steps=1000, decay_rate=0.99, staircase=False):
    """run_gnn.py:275-288 (pure arithmetic)"""
    if lr_type == "constant":
        return float(lr)
    if lr_type == "fixed_decay":                 # tf.train.exponential_decay
        p = global_step / float(decay_steps)
        return lr * decay_rate ** (math.floor(p) if staircase else p)
    if lr_type == "polynomial_decay":            # tf.train.polynomial_decay, cycle=False
        end = lr / 100.0
        s = min(global_step, num_train_iters)
        return (lr - end) * (1.0 - s / float(num_train_iters)) ** 0.5 + end
    raise ValueError(f"lr_type={lr_type!r}")


def encoder_trainer_state(tr):
    """What a resumed encoder run needs: parameters, Adam moments, step counter, the batch norms' moving statistics."""
    return _state(tr, tr.net.bns)


def load_encoder_trainer_state(tr, state):
    """Restore encoder_trainer_state's dict into a connected trainer."""
    _load_state(tr, tr.net.bns, state, "encoder")
