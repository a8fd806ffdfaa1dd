"""The encoder's training step without a GPU: the C ABI of include/gnf_timestep_gnn_train.h is in step with the library and the
binding; the autograd restatement the GPU tests compare against (tests/timestep_gnn_grad_ref.py) agrees with central finite
differences in float64; the learning-rate schedules of run_gnn.py:275-288 in closed form; and every GPU case has inputs that
satisfy the restatement's seed condition, so that no GPU case is ever skipped for want of a seed."""
import math
import os
import re

import numpy as np
import pytest

from gnf_amd import _abi
from gnf_amd.train import encoder_learning_rate

import timestep_gnn_grad_ref as G
import timestep_gnn_ref as R

NEW_SYMBOLS = ("gnf_timestep_gnn_stash_bytes", "gnf_timestep_gnn_train_forward_f32", "gnf_timestep_gnn_backward_workspace_bytes",
               "gnf_timestep_gnn_backward_f32")


def test_header_library_and_binding_agree():
    """include/gnf_timestep_gnn_train.h (included by gnf.h behind gnf_timestep_gnn.h), the library's exports and
    _abi.ENCODER_TRAIN_SYMBOLS are in step, and the new table shares nothing with the others"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_timestep_gnn_train.h"$', main, flags=re.M)
    assert main.index('#include "gnf_timestep_gnn.h"') < main.index('#include "gnf_timestep_gnn_train.h"')
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_timestep_gnn_train.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.ENCODER_TRAIN_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS):
        assert not set(_abi.ENCODER_TRAIN_SYMBOLS) & set(other)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.gnf_abi_version() == 10


def test_size_functions_return_zero_for_arguments_no_call_accepts():
    import ctypes as C
    lib = _abi.lib()
    assert lib.gnf_timestep_gnn_stash_bytes(10, 6, None) == 0 and lib.gnf_timestep_gnn_backward_workspace_bytes(10, 6, None) == 0
    nets = (_abi.GnfMlp * 1)()
    nets[0].num_layers, nets[0].dims[0], nets[0].dims[1] = 1, 6, 6
    g = _abi.GnfTimestepGnn(2, 1, C.cast(nets, C.POINTER(_abi.GnfMlp)), _abi.GnfGnnSpec(0, 0, 1.0, 0, 0.2), None, None, 1, 1, 0,
                            1e-3, 0.999)
    for fn in (lib.gnf_timestep_gnn_stash_bytes, lib.gnf_timestep_gnn_backward_workspace_bytes):
        assert fn(-1, 6, C.byref(g)) == 0 and fn(10, 0, C.byref(g)) == 0 and fn(10, 6, C.byref(g)) > 0
    # T = 2 without norms: one [n, D] buffer of rows (the module input of timestep 1), rounded up to 64 floats
    assert lib.gnf_timestep_gnn_stash_bytes(10, 6, C.byref(g)) == 64 * 4
    assert lib.gnf_timestep_gnn_stash_bytes(1000, 6, C.byref(g)) == (6000 + 63) // 64 * 64 * 4


# ---- the reference against finite differences ---------------------------------------------------------------------------------
FD_SIZES = [4, 1, 2]   # 7 nodes: a ring with both directions, a self loop, a two-node graph


@pytest.mark.parametrize("family,sharing", [("avg", False), ("sumcat", True)])
def test_autograd_reference_agrees_with_central_differences(family, sharing):
    c = G.Case(family, 3, 5, 3, 2, True, True, True, sharing)
    batch = R.ring_chord_batch(FD_SIZES, edgeless=())
    rng = np.random.default_rng(11)
    x = rng.standard_normal((7, c.d))
    g_out = rng.standard_normal((7, c.d))
    params = G.make_params(c)
    kw = G.FAMILY_KW[family]

    def value(p, xx):
        return float((G.train_step(batch, xx, p, c.t, np.float64, kw, sharing, True, g_out=np.zeros_like(g_out))["out"] * g_out).sum())
    ref = G.train_step(batch, x, params, c.t, np.float64, kw, sharing, True, g_out=g_out)
    assert G.R.margin_ok(ref["pre"], {k: v + 1e-5 for k, v in ref["pre"].items()})   # no hidden unit within 4e-5 of a kink: h = 1e-6 is safe
    flat = G.flatten(ref["grads"], ref["g_x"])
    h = 1e-6
    checked = set()
    for name, grad in flat.items():
        fam = re.sub(r"\d+", "", name)
        idx = [tuple(int(v) for v in np.unravel_index(k, grad.shape)) for k in rng.choice(grad.size, size=min(4, grad.size), replace=False)]
        for ix in idx:
            def bumped(delta):
                p = {k: [([(w.astype(np.float64).copy(), b.astype(np.float64).copy()) for (w, b) in net] if k == "nets" else
                          {kk: np.asarray(vv, np.float64).copy() for kk, vv in net.items()}) for net in v] for k, v in params.items()}
                xx = x.copy()
                if name == "g_x":
                    xx[ix] += delta
                else:
                    m = re.match(r"(net|bn|ln)(\d+)\.(\w+?)(\d*)$", name)
                    kind, q, key, j = m.group(1), int(m.group(2)), m.group(3), m.group(4)
                    if kind == "net":
                        p["nets"][q][int(j)][0 if key == "W" else 1][ix] += delta
                    else:
                        p[kind][q][key][ix] += delta
                return value(p, xx)
            fd = (bumped(h) - bumped(-h)) / (2 * h)
            assert abs(fd - grad[ix]) <= 1e-6 * max(1.0, abs(grad[ix])), (name, ix, fd, grad[ix])
        checked.add(fam)
    assert checked == {"net.W", "net.b", "bn.gamma", "bn.beta", "ln.gamma", "ln.beta", "g_x"}


def test_batch_norm_backward_formula_of_the_header():
    """du = gamma rsqrt(var + eps) (g - dbeta / N - u^ dgamma / N): the header's closed form against autograd, and du = 0 at N = 1"""
    import torch
    rng = np.random.default_rng(3)
    for n in (1, 5):
        u = torch.tensor(rng.standard_normal((n, 4)), requires_grad=True)
        gamma, beta = torch.tensor(rng.uniform(0.5, 1.5, 4), requires_grad=True), torch.tensor(rng.standard_normal(4), requires_grad=True)
        g = torch.tensor(rng.standard_normal((n, 4)))
        y, mean, var = R.batch_norm(u, {"gamma": gamma, "beta": beta}, True)
        (y * g).sum().backward()
        rs = torch.rsqrt(var + R.BN_EPS).detach()
        uh = (u.detach() - mean.detach()) * rs
        dbeta, dgamma = g.sum(0), (g * uh).sum(0)
        du = gamma.detach() * rs * (g - dbeta / n - uh * dgamma / n)
        assert torch.allclose(du, u.grad, atol=1e-12) and torch.allclose(dbeta, beta.grad) and torch.allclose(dgamma, gamma.grad)
        if n == 1:
            assert float(du.abs().max()) == 0.0


# ---- learning-rate schedules ----------------------------------------------------------------------------------------------------
def test_learning_rate_schedules_in_closed_form():
    lr = 1e-4
    for step in (0, 1, 1000, 5000):
        assert encoder_learning_rate("constant", lr, step) == lr
        want = lr * 0.99 ** (step / 1000.0)
        assert math.isclose(encoder_learning_rate("fixed_decay", lr, step, decay_steps=1000, decay_rate=0.99), want, rel_tol=1e-15)
        stair = lr * 0.99 ** (step // 1000)
        assert math.isclose(encoder_learning_rate("fixed_decay", lr, step, decay_steps=1000, decay_rate=0.99, staircase=True), stair,
                            rel_tol=1e-15)
    assert encoder_learning_rate("fixed_decay", lr, 999, decay_steps=1000, staircase=True) == lr
    n = 2000
    for step, frac in ((0, 1.0), (1, 1.0 - 1.0 / n), (n, 0.0), (n + 7, 0.0), (10 * n, 0.0)):
        want = (lr - lr / 100.0) * math.sqrt(frac) + lr / 100.0
        assert math.isclose(encoder_learning_rate("polynomial_decay", lr, step, num_train_iters=n), want, rel_tol=1e-14), step
    assert encoder_learning_rate("polynomial_decay", lr, 0, num_train_iters=n) == lr
    assert math.isclose(encoder_learning_rate("polynomial_decay", lr, n, num_train_iters=n), lr / 100.0, rel_tol=1e-15)
    with pytest.raises(ValueError):
        encoder_learning_rate("schedule", lr, 0)


def test_trainer_schedule_follows_its_step_counter():
    from gnf_amd.train import EncoderTrainer
    tr = EncoderTrainer(None, lr=2e-4, num_train_iters=100)
    assert tr.current_learning_rate() == 2e-4
    tr.global_step = 100
    assert math.isclose(tr.current_learning_rate(), 2e-6, rel_tol=1e-15)
    tr = EncoderTrainer(None, lr=2e-4, lr_type="fixed_decay", lr_fixed_decay_steps=10, lr_fixed_decay_rate=0.5)
    tr.global_step = 20
    assert math.isclose(tr.current_learning_rate(), 5e-5, rel_tol=1e-15)
    with pytest.raises(ValueError):
        EncoderTrainer(None, lr_type="schedule")


# ---- every GPU case has its inputs ----------------------------------------------------------------------------------------------
def test_the_cases_cover_every_value_in_both_families():
    for fam in ("avg", "sumcat"):
        cs = [c for c in G.GRAD_CASES if c.family == fam]
        assert {c.d for c in cs} == {6, 100} and {c.k for c in cs} == {1, 2, 3} and {c.t for c in cs} == {1, 3}
        assert {(c.bn, c.ln) for c in cs} == {(False, False), (True, False), (False, True), (True, True)}
        assert {c.residual for c in cs} == {False, True} and {c.sharing for c in cs} == {False, True}
    assert {c.family for c in G.GRAD_CASES} == {"avg", "sumcat", "sum", "meancat"} and len(G.GRAD_CASES) == 16


@pytest.mark.parametrize("c", G.GRAD_CASES, ids=R.case_id)
def test_every_gradient_case_has_a_seed(c):
    seed, x, r64, r32 = G.pick_seed(c)
    assert seed is not None, "no seed in range(16) keeps every hidden unit 4 float32 deviations from its kink: change the case"
    assert max(float(np.abs(v).max()) for v in G.flatten(r64["grads"], r64["g_x"]).values()) > 1e-3


@pytest.mark.parametrize("kind", G.E2E_KINDS)
def test_every_end_to_end_case_has_a_seed_and_few_clipped_pairs(kind):
    seed, x, r64, r32 = G.pick_e2e(kind)
    assert seed is not None
    # a case dominated by pairs inside Keras' clip (no gradient there) would test nothing
    assert r64["clipped"] <= 8 and r64["pairs"] == 1570 and r64["clip_gap"] >= G.CLIP_GAP
    assert float(np.abs(r64["g_out"]).max()) > 1e-2
