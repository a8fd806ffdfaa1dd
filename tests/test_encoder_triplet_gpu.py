"""train.EncoderTrainer(loss_type="triplet") and examples/run_gnn.py --loss_type triplet on the MI355X.

The gradient of every encoder variable is held against tests/timestep_gnn_grad_ref.train_step in float64 under that file's
`compare`, with the triplet restatement (tests/triplet_loss_ref.py, same seed) as the loss behind the encoder: train_step takes
an upstream dL/d out, so the reference runs it twice - once for the encoder's output, then with the restatement's gradient at
that output.  The inputs are the first seed in range(16) with timestep_gnn_ref.margin_ok on the hidden units and
triplet_loss_ref.margin_ok on the terms, the float32 run's scores taken at the float32 encoder output (so the gap covers what
the encoder's own fp32 error moves a score by).  Every figure is printed before it is asserted (pytest -s)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gnf_amd import encoder
from gnf_amd.train import EncoderTrainer
from helpers import graph_from_arrays

import timestep_gnn_grad_ref as G
import timestep_gnn_ref as R
import triplet_loss_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"l2-margin": (G.GRAD_CASES[0], T.L2, T.MARGIN, 8), "cauchy-relative": (G.GRAD_CASES[4], T.CAUCHY, T.RELATIVE, 3)}
HASH_SEED = 21


def _tokens(score, loss):
    from gnf_amd.triplet_loss import hacky_cauchy_l2, l2, margin_loss, relative_loss
    return (l2 if score == T.L2 else hacky_cauchy_l2), (margin_loss(loss[1]) if loss[0] == "margin" else relative_loss)


@functools.lru_cache(maxsize=None)
def _pick(key):
    """(seed, x, ref64, ref32, loss64, loss32) of a case; cached: callers must not change the references"""
    c, score, loss, loops = CASES[key]
    params = G.make_params(c)
    nn, _, s, r = R.ring_chord_batch(R.SIZES)
    sizes = [int(v) for v in nn]
    for seed in range(16):
        x = R.module_inputs(c, seed)
        idx = T.sample(sizes, s, r, T.hash_draws(HASH_SEED, loops, len(x)))
        runs = []
        for dtype in (np.float64, np.float32):
            out = G.run_case(c, x, dtype, params, g_out=np.zeros_like(x))["out"]
            tl = T.triplet_loss(out, sizes, s, r, score, loss, indices=idx, dtype=dtype)
            runs.append((G.run_case(c, x, dtype, params, g_out=tl["grad"]), tl))
        (r64, l64), (r32, l32) = runs
        if R.margin_ok(r64["pre"], r32["pre"]) and T.margin_ok(l64, l32):
            return seed, x, r64, r32, l64, l32
    return None, None, None, None, None, None


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _graph(x):
    nn, ne, s, r = R.ring_chord_batch(R.SIZES)
    return graph_from_arrays(nn, ne, s, r, x, DEV)


def _encoder(c):
    return encoder.make_encoder(G.family_hp(c)).set_params(G.make_params(c))


@pytest.mark.parametrize("key", list(CASES))
def test_loss_and_grads_against_the_restatement_behind_the_reference(key):
    seed, x, r64, r32, l64, l32 = _pick(key)
    assert seed is not None, "no seed in range(16) satisfies both margin conditions"
    c, score, loss, loops = CASES[key]
    fn, lf = _tokens(score, loss)
    tr = EncoderTrainer(_encoder(c), loss_type="triplet", triplet_dist_fn=fn, triplet_loss_fn=lf, num_sampling_loops=loops,
                        seed=HASH_SEED)
    res = tr.loss_and_grads(_graph(x))
    torch.cuda.synchronize()
    assert np.array_equal(res["skipped_terms"].cpu().numpy(), l64["skipped"])
    total, bound = float(res["total_loss"]), T.bounds(l64, l32)["sum_loss"]
    print(f"[encoder-triplet] {key}: total_loss {total:.6f} reference {l64['sum_loss']:.6f} bound {bound:.3e}")
    assert abs(total - l64["sum_loss"]) <= bound and total == float(res["sum_loss"]) and l64["sum_loss"] > 0
    assert abs(float(res["loss_per_node"].sum()) - total) <= 1e-5 * total
    assert res["false_positive_pairs"].shape == res["false_negative_pairs"].shape == (len(R.SIZES),)
    assert res["gnn_output"].nodes.shape == x.shape
    got = G.flatten(tr.named_gradients())
    worst, bad = G.compare(f"triplet {key}", got, r64, r32)
    assert not bad, "\n".join(bad)
    assert tr.grad.numel() == sum(v.size for v in got.values()) and max(float(np.abs(v).max()) for v in got.values()) > 0


def test_three_adam_steps_lower_the_loss_on_fixed_draws():
    c = G.GRAD_CASES[0]
    x = R.module_inputs(c, 0)
    graph = _graph(x)
    draws = torch.as_tensor(T.hash_draws(5, 8, len(x)).astype(np.int64)).to(DEV)
    tr = EncoderTrainer(_encoder(c), loss_type="triplet", lr=1e-3, lr_type="constant", draws=draws)
    losses = [float(tr.step(graph)["total_loss"]) for _ in range(3)]
    losses.append(float(tr.loss_and_grads(graph)["total_loss"]))
    print(f"[encoder-triplet] losses over three Adam steps: {losses}")
    assert tr.global_step == 3 and all(np.isfinite(losses)) and losses[3] < losses[0]
    # without `draws` the samples are those of seed + global_step: another step, other samples
    a = EncoderTrainer(_encoder(c), loss_type="triplet", seed=3)
    b = EncoderTrainer(_encoder(c), loss_type="triplet", seed=3)
    la, lb = float(a.loss_and_grads(graph)["total_loss"]), float(b.loss_and_grads(graph)["total_loss"])
    b.global_step = 1
    assert la == lb and float(b.loss_and_grads(graph)["total_loss"]) != lb


def test_tune_sigmoid_with_the_triplet_loss_is_a_value_error():
    from gnf_amd import adj_loss
    with pytest.raises(ValueError):
        EncoderTrainer(_encoder(G.GRAD_CASES[0]), loss_type="triplet", tune_sigmoid=True, distance_fn=adj_loss.sigmoid_l2(10.0, 1.0))
    with pytest.raises(ValueError):
        EncoderTrainer(_encoder(G.GRAD_CASES[0]), loss_type="triplet", tune_sigmoid=True, distance_fn=adj_loss.TunedSigmoidL2())


def test_the_example_trains_on_the_triplet_loss(tmp_path):
    path = str(tmp_path / "encoder.npz")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_gnn.py"), "--dataset", "graph_rnn_grid_small",
                          "--loss_type", "triplet", "--triplet_loss_fn", "relative", "--triplet_dist_fn", "hacky_sigmoid_l2",
                          "--node_embedding_dim", "6", "--latent_dim", "16", "--num_layers", "2", "--num_processing_steps", "2",
                          "--train_batch_size", "4", "--num_train_iters", "3", "--log_every_n_steps", "1",
                          "--eval_every_n_steps", "2", "--save_path", path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "iteration num: 2" in run.stdout and "after 3 steps" in run.stdout and "triplet terms without a candidate:" in run.stdout
    losses = [float(line.split(":")[1]) for line in run.stdout.splitlines() if line.startswith("sum loss:")]
    assert len(losses) == 3 and all(np.isfinite(losses)) and all(v > 0 for v in losses)
    enc, hp = encoder.load_encoder(path)
    assert hp["node_dim"] == 6 and encoder.distance_of(hp).__name__ == "hacky_sigmoid_l2"
