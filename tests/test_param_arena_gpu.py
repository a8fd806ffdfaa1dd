"""Where every trainable variable lives: the layout of the trainers' flat vectors (train.GRevNetTrainer, train.EncoderTrainer).

theta is the concatenation of the trainable tensors in one fixed order, every live parameter tensor is a view of theta at its
offset, and named_gradients() cuts grad at the same offsets.  The order:
  GRevNetTrainer   the MLPs of s then t (index half * T + i), (W, b) per layer; the attention blocks of s then t over
                   attn_keys(); the batch-norm bijectors' gamma, beta at index half * T + i
  EncoderTrainer   the nets' (W, b) per layer; the batch norms' gamma, beta per timestep; the layer norms'; with tune_sigmoid
                   the distance function's temp, shift as the last two entries
A mismatch here raises no error anywhere else - it sends a gradient to the wrong variable - so the comparisons are bitwise.
The same holds after set_params with new values (the arena is re-seated on them), and Adam's moments keep their storage then."""
import numpy as np
import pytest
import torch

from gnf_amd import adj_loss, encoder
from gnf_amd.factories import make_product_grevnet
from gnf_amd.train import EncoderTrainer, GRevNetTrainer
from helpers import graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, LATENT, K, T = 4, 8, 2, 2
MP = dict(activation="leaky_relu", agg="mean", combine="agg", epsilon=2.0)

FLOWS = {
    "avg_then_mlp": dict(MP, weight_sharing=False),
    "sum_concat_shared_bn": dict(MP, agg="sum", combine="concat", weight_sharing=True, use_batch_norm=True),
    "dm_self_attn_ln_bn": dict(activation="relu", weight_sharing=False, use_batch_norm=True,
                               attn=dict(num_heads=2, kq_dim=3, v_dim=5, out_dim=6, concat=True, kq_dim_division=True,
                                         residual=False, layer_norm=True)),
    "self_attn": dict(activation="relu", weight_sharing=False, attn=dict(scope="graph", kq_dim=3, v_dim=5)),
}
ENCODERS = {
    "bn_ln": dict(use_batch_norm=True, use_layer_norm=True),
    "bn_ln_shared": dict(use_batch_norm=True, use_layer_norm=True, weight_sharing=True),
    "bn_ln_shared_tune_sigmoid": dict(use_batch_norm=True, use_layer_norm=True, weight_sharing=True, tune_sigmoid=True),
    "plain_tune_sigmoid": dict(tune_sigmoid=True),
}


def _graph():
    """two graphs of 3 and 5 nodes: a directed ring each, both ways, and one chord in the second"""
    s, r = [], []
    for off, n in ((0, 3), (3, 5)):
        for i in range(n):
            s += [off + i, off + (i + 1) % n]
            r += [off + (i + 1) % n, off + i]
    s, r = s + [3], r + [6]
    x = np.random.default_rng(7).standard_normal((8, D)).astype(np.float32)
    return graph_from_arrays([3, 5], [6, 11], s, r, x, DEV)


def _flow_order(net, container):
    """[(name, value)] of a container in GRevNet.get_params()'s layout (or named_gradients()'), in arena order"""
    flat = {kind: list(container[kind]) if net.weight_sharing else list(container[kind][0]) + list(container[kind][1])
            for kind in ("s", "t")}
    out = []
    for kind in ("s", "t"):
        for q, one in enumerate(flat[kind]):
            for j, (w, b) in enumerate(one["mlp"] if isinstance(one, dict) else one):
                out += [(f"{kind}{q}.W{j}", w), (f"{kind}{q}.b{j}", b)]
    for kind in ("s", "t"):
        for q, (blk, one) in enumerate(zip(net.blocks(kind), flat[kind])):
            if isinstance(one, dict):
                out += [(f"{kind}{q}.attn.{k}", one["attn"][k]) for k in blk.attn_keys()]
    for half, bns in enumerate(container.get("bn") or []):
        for i, d in enumerate(bns):
            out += [(f"bn{half}.{i}.gamma", d["gamma"]), (f"bn{half}.{i}.beta", d["beta"])]
    return out


def _flow_live(net):
    """the live device tensors in the same order"""
    out = []
    for kind in ("s", "t"):
        out += [t for m in net.mlps(kind) for wb in m.params for t in wb]
    for blk in net.blocks("s") + net.blocks("t"):
        if getattr(blk, "attn_params", None) is not None:
            out += [blk.attn_params[k] for k in blk.attn_keys()]
    if net.use_batch_norm:
        out += [t for half in net.bns for b in half for t in (b.gamma, b.beta)]
    return out


def _encoder_order(container):
    out = []
    for q, one in enumerate(container["nets"]):
        for j, (w, b) in enumerate(one):
            out += [(f"net{q}.W{j}", w), (f"net{q}.b{j}", b)]
    for key in ("bn", "ln"):
        for i, d in enumerate(container.get(key) or []):
            out += [(f"{key}{i}.gamma", d["gamma"]), (f"{key}{i}.beta", d["beta"])]
    return out


def _encoder_live(enc):
    out = [t for b in enc.blocks() for wb in b._mlp.params for t in wb]
    return out + [t for o in list(enc.bns) + list(enc.lns) for t in (o.gamma, o.beta)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def _check_layout(tr, params, grads, live, trailing=0):
    """the three properties; returns the number of entries the containers account for"""
    torch.cuda.synchronize()
    theta, grad = tr.theta.detach().cpu().numpy(), tr.grad.detach().cpu().numpy()
    assert theta.dtype == np.float32 and theta.ndim == 1 and grad.shape == theta.shape
    assert [n for n, _ in params] == [n for n, _ in grads] and len(params) == len(live)
    off = 0
    for (name, p), (_, g), t in zip(params, grads, live):
        size = int(np.asarray(p).size)
        assert tuple(np.asarray(p).shape) == tuple(np.asarray(g).shape) == tuple(t.shape), name
        assert np.array_equal(_bits(theta[off:off + size]), _bits(p)), f"theta: {name} at {off}"
        assert t.data_ptr() == tr.theta.data_ptr() + 4 * off and t.is_contiguous(), f"{name} is not theta's entry {off}"
        assert np.array_equal(_bits(grad[off:off + size]), _bits(g)), f"grad: {name} at {off}"
        off += size
    assert off + trailing == theta.size
    return off


def _perturbed(tree, rng):
    """the same container with new values (the moving statistics included)"""
    if isinstance(tree, dict):
        return {k: _perturbed(v, rng) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_perturbed(v, rng) for v in tree)
    a = np.asarray(tree, np.float32)
    return (a + 0.05 * rng.standard_normal(a.shape) + 0.01).astype(np.float32)


@pytest.mark.parametrize("case", list(FLOWS), ids=list(FLOWS))
def test_flow_trainer_layout(case):
    hp = dict(FLOWS[case], D=D, latent=LATENT, K=K, T=T)
    net = make_product_grevnet(hp)
    tr = GRevNetTrainer(net, lr=1e-2)
    graph = _graph()
    tr.loss_and_grads(graph)
    total = _check_layout(tr, _flow_order(net, net.get_params()), _flow_order(net, tr.named_gradients()), _flow_live(net))
    assert float(np.abs(tr.grad.cpu().numpy()).max()) > 0.0
    m_ptr, v_ptr = tr.m.data_ptr(), tr.v.data_ptr()
    new = _perturbed(net.get_params(), np.random.default_rng(11))
    net.set_params(new)
    tr.step(graph)
    assert _check_layout(tr, _flow_order(net, net.get_params()), _flow_order(net, tr.named_gradients()), _flow_live(net)) == total
    assert (tr.m.data_ptr(), tr.v.data_ptr()) == (m_ptr, v_ptr)
    # the step started from the new values: one Adam step of size <= lr moves no entry further than that
    moved = np.concatenate([np.asarray(a).ravel() for _, a in _flow_order(net, new)]) - tr.theta.cpu().numpy()
    assert float(np.abs(moved).max()) <= 1.01e-2   # (lr 1e-2; the bijectors' gamma projection adds 1e-6)


@pytest.mark.parametrize("case", list(ENCODERS), ids=list(ENCODERS))
def test_encoder_trainer_layout(case):
    kw = dict(ENCODERS[case])
    tune = kw.pop("tune_sigmoid", False)
    enc = encoder.make_encoder(dict(MP, node_dim=D, latent=LATENT, K=K, num_timesteps=T, **kw))
    tr = EncoderTrainer(enc, lr=1e-2, lr_type="constant", max_nodes_per_graph=8, tune_sigmoid=tune,
                        distance_fn=adj_loss.sigmoid_l2(3.0, 2.0) if tune else None)
    graph = _graph()
    tr.loss_and_grads(graph)
    trailing = 2 if tune else 0
    total = _check_layout(tr, _encoder_order(enc.get_params()), _encoder_order(tr.named_gradients()), _encoder_live(enc), trailing)
    if tune:   # temp, shift: the last two entries, and distance_fn.params is a view of them
        assert tr.distance_fn.params.data_ptr() == tr.theta.data_ptr() + 4 * total
        assert tr.theta[-2:].cpu().tolist() == [3.0, 2.0]
    m_ptr, v_ptr = tr.m.data_ptr(), tr.v.data_ptr()
    new = _perturbed(enc.get_params(), np.random.default_rng(12))
    enc.set_params(new)
    tr.step(graph)
    assert _check_layout(tr, _encoder_order(enc.get_params()), _encoder_order(tr.named_gradients()), _encoder_live(enc),
                         trailing) == total
    assert (tr.m.data_ptr(), tr.v.data_ptr()) == (m_ptr, v_ptr)
    if tune:
        assert tr.distance_fn.params.data_ptr() == tr.theta.data_ptr() + 4 * total
        assert float(np.abs(tr.theta[-2:].cpu().numpy() - np.float32([3.0, 2.0])).max()) <= 1.01e-2
    moved = np.concatenate([np.asarray(a).ravel() for _, a in _encoder_order(new)]) - tr.theta[:total].cpu().numpy()
    assert float(np.abs(moved).max()) <= 1.01e-2
