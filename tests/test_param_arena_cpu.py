"""params.ParamArena on plain CPU tensors and dummy owners: the layout both trainers' flat vectors come from (the trainers
themselves on the device: tests/test_param_arena_gpu.py)."""
import torch

from gnf_amd.params import ParamArena, read, write


class _Owner:
    pass


def _owners():
    """the three slot shapes the trainers use: a list of (W, b) tuples, a dict, plain attributes"""
    g = torch.Generator().manual_seed(3)
    mlp, attn, norm = _Owner(), _Owner(), _Owner()
    mlp.params = [(torch.randn(3, 5, generator=g), torch.randn(5, generator=g)),
                  (torch.randn(5, 2, generator=g), torch.randn(2, generator=g))]
    attn.attn_params = {"wq": torch.randn(3, 4, generator=g), "ln_gamma": torch.ones(2)}
    norm.gamma, norm.beta = torch.full((7,), 1.5), torch.zeros(7)
    slots = [(mlp, "params", j, h) for j in range(2) for h in (0, 1)]
    slots += [(attn, "attn_params", "wq"), (attn, "attn_params", "ln_gamma"), (norm, "gamma"), (norm, "beta")]
    return (mlp, attn, norm), slots


def test_read_and_write_reach_every_slot_shape():
    (mlp, attn, norm), slots = _owners()
    assert read(slots[1]) is mlp.params[0][1] and read(slots[4]) is attn.attn_params["wq"] and read(slots[6]) is norm.gamma
    params, d = mlp.params, attn.attn_params
    new = [torch.zeros_like(read(s)) for s in slots]
    for s, t in zip(slots, new):
        write(s, t)
    assert all(read(s) is t for s, t in zip(slots, new))
    assert mlp.params is params and attn.attn_params is d                  # the owners' containers are kept
    assert all(type(p) is tuple and len(p) == 2 for p in mlp.params) and list(d) == ["wq", "ln_gamma"]


def test_layout_bounds_and_views_put_back():
    (mlp, attn, norm), slots = _owners()
    before = [read(s).clone() for s in slots]
    arena = ParamArena().seat(slots, "cpu")
    sizes = [15, 5, 10, 2, 12, 2, 7, 7]
    assert arena.bounds == [sum(sizes[:i]) for i in range(len(sizes) + 1)]
    assert arena.offsets.dtype == torch.int64 and arena.offsets.tolist() == arena.bounds
    assert arena.theta.dtype == torch.float32 and arena.theta.shape == (60,) and arena.tail.numel() == 0
    assert torch.equal(arena.theta, torch.cat([t.reshape(-1) for t in before]))
    for s, old, view, off in zip(slots, before, arena.views, arena.bounds):
        assert read(s) is view and view.shape == old.shape and torch.equal(view, old)
        assert view.data_ptr() == arena.theta.data_ptr() + 4 * off
    arena.theta.add_(1.0)                                                  # an optimiser step is seen through the owners
    assert torch.equal(norm.gamma, torch.full((7,), 2.5)) and torch.equal(mlp.params[1][0], before[2] + 1.0)


def test_gradient_views_alias_grad():
    _, slots = _owners()
    arena = ParamArena().seat(slots, "cpu")
    assert arena.grad.shape == arena.theta.shape and not arena.grad.any()
    for i, (view, gview, off) in enumerate(zip(arena.views, arena.grad_views, arena.bounds)):
        assert gview.shape == view.shape and gview.data_ptr() == arena.grad.data_ptr() + 4 * off
        gview.fill_(float(i + 1))
    want = torch.cat([torch.full((b - a,), float(i + 1)) for i, (a, b) in enumerate(zip(arena.bounds, arena.bounds[1:]))])
    assert torch.equal(arena.grad, want)


def test_moments_are_kept_by_size_and_dropped_otherwise():
    (mlp, attn, norm), slots = _owners()
    arena = ParamArena().seat(slots, "cpu")
    assert not arena.m.any() and not arena.v.any() and arena.m.data_ptr() != arena.v.data_ptr()
    arena.m.fill_(3.0), arena.v.fill_(4.0)
    m, v, theta = arena.m, arena.v, arena.theta
    norm.gamma = torch.full((7,), -2.0)                                    # a set_params: same size, new tensor
    arena.seat(slots, "cpu")
    assert arena.m is m and arena.v is v and arena.theta is not theta
    assert norm.gamma is arena.views[6] and torch.equal(arena.theta[46:53], torch.full((7,), -2.0))
    assert torch.equal(arena.theta[:46], theta[:46])                       # the other values came over from the old views
    norm.gamma, norm.beta = torch.ones(8), torch.zeros(8)                  # another size: fresh moments
    arena.seat(slots, "cpu")
    assert arena.m is not m and arena.m.shape == (62,) and not arena.m.any() and not arena.v.any()


def test_trailing_entries():
    _, slots = _owners()
    arena = ParamArena().seat(slots, "cpu", trailing=2)
    assert arena.theta.shape == arena.grad.shape == arena.m.shape == (62,) and arena.bounds[-1] == 60
    assert len(arena.views) == len(slots) and arena.offsets.tolist() == arena.bounds
    assert arena.tail.shape == (2,) and arena.tail.data_ptr() == arena.theta.data_ptr() + 4 * 60
    assert arena.grad_tail.shape == (2,) and arena.grad_tail.data_ptr() == arena.grad.data_ptr() + 4 * 60
    arena.tail.copy_(torch.tensor([3.0, 2.0]))
    assert arena.theta[-2:].tolist() == [3.0, 2.0]


def test_is_seated_compares_one_integer_then_every_owner():
    (mlp, attn, norm), slots = _owners()
    arena = ParamArena()
    assert not arena.is_seated("cpu", 0)
    arena.seat(slots, "cpu")
    assert arena.epoch is None and arena.is_seated("cpu", 5) and arena.epoch == 5      # full check passed: epoch recorded
    kept = attn.attn_params["wq"]
    attn.attn_params = dict(attn.attn_params, wq=kept.clone())             # re-bound outside the arena ...
    assert arena.is_seated("cpu", 5)                                       # ... unseen while the epoch stands
    assert not arena.is_seated("cpu", 6) and arena.epoch == 5
    attn.attn_params["wq"] = kept
    assert arena.is_seated("cpu", 6) and arena.epoch == 6
    mlp.params[0] = (mlp.params[0][0], mlp.params[0][1].clone())
    assert not arena.is_seated("cpu", 7)
    assert not ParamArena().seat(slots, "cpu").is_seated("meta", 0)        # another device: never seated
