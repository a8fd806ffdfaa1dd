"""Prologue and epilogue of the phased compile-time-geometry half-step kernel (k_half_fused_geo<.., PHASES = true>,
gnf_fused.hip): the two nets' bias blocks reach the waves through an LDS block behind the col slice, every wave takes the
col segment's bounds from its own rowptr registers (no barrier in front of the col request), and the wave sums of s and
x_new^2 are reduced in registers.  None of it may change a bit: every case is a three-way torch.equal of automatic
dispatch, force_shape = 13 (one net per wave, biases from global memory) and force_shape = 12 (the generic kernel, the
`__shfl_down` reduction) on z, on [logdet, sum z^2] and on the inverse's x - D = 64, L = 256, K = 5, T = 2 with unshared
weights through the public flow entry point, so consecutive launches bring different bias blocks and the last two carry
the sum of squares.

  biases: every (half-step, net, layer, column) has its own non-zero value (set by the test, exact in float32); N = 1, 16,
      17, 47 over three graphs, mean + leaky_relu and sum + relu, one strided misaligned layout.
  zero weights: every weight matrix is zero, so s and t are functions of the biases alone and a bias column that reaches
      the wrong accumulator cannot hide in rounding.
  col segments: N = 17; the first tile's segment has 0 / 1 / 511 / 512 / 513 / 2 048 / 2 049 entries (the kernel's own
      first request covers 512; the LDS slice in front of the bias block holds 2 048; 2 049 stay in global memory).
  an isolated node and degrees 9 - 17 (two and three gather rounds).
  two runs in one process with workspace and destination refilled with NaN in between."""
import numpy as np
import pytest

from oracle import gnf_oracle as O
from test_fused_geo_gpu import (D, K, L, LAYOUTS, NETS, T, _hp, _problem, _require_gpu_and_native_lib,  # noqa: F401
                                force_shape)
from test_fused_geo_phases_gpu import AUTO, GENERIC, PARENT, _assert_same, _run

pytestmark = pytest.mark.gpu


N_BIAS = 2 * 2 * T * ((K - 1) * L + D // 2)   # nets x halves x timesteps x (hidden layers + output layer)


def _with_distinct_biases(pr, weights=lambda w: w):
    """A copy of the problem whose biases are +-(2^-6 + q 2^-17), q a permutation of 0 .. N_BIAS - 1 over every (net, half,
    timestep, layer, column), the sign alternating with q: exact in float32, non-zero, no two equal, |b| < 0.09."""
    q = np.random.default_rng(N_BIAS).permutation(N_BIAS)
    vals = ((2.0 ** -6 + q * 2.0 ** -17) * np.where(q & 1, -1.0, 1.0)).astype(np.float32)
    assert np.all(vals != 0) and np.unique(vals).size == N_BIAS
    at = [0]

    def take(b):
        out = vals[at[0]:at[0] + b.size].reshape(b.shape)
        at[0] += b.size
        return out
    p = {name: [[[(weights(w), take(b)) for w, b in mlp] for mlp in half] for half in pr["p"][name]] for name in ("s", "t")}
    assert at[0] == N_BIAS
    return dict(pr, p=p)


def _three_way(pr, layout, force_shape, weights=lambda w: w):
    pr = _with_distinct_biases(pr, weights)
    auto, parent, generic = _run(pr, layout, force_shape, (AUTO, PARENT, GENERIC))
    _assert_same(auto, generic, "automatic dispatch vs force_shape = 12")
    _assert_same(parent, generic, "force_shape = 13 vs force_shape = 12")
    _assert_same(auto, parent, "automatic dispatch vs force_shape = 13")


@pytest.mark.parametrize("net", ["mean_leaky", "sum_relu"])
@pytest.mark.parametrize("gname", ["n1", "n16_one_graph", "n17_two_graphs", "n47_three_graphs", "isolated_and_deg9to17"])
def test_distinct_biases_three_way(force_shape, gname, net):
    _three_way(_problem(gname, *NETS[net]), LAYOUTS["contiguous"], force_shape)


def test_distinct_biases_on_strided_misaligned_rows(force_shape):
    _three_way(_problem("n47_three_graphs", *NETS["sum_relu"]), LAYOUTS["ldD+3_c3"], force_shape)


@pytest.mark.parametrize("net", ["mean_leaky", "sum_relu"])
def test_zero_weights_output_is_the_biases_alone(force_shape, net):
    # (with W = 0 every row of a half-step gets the same s and t, K layers of biases and activations and nothing else)
    _three_way(_problem("n47_three_graphs", *NETS[net]), LAYOUTS["contiguous"], force_shape, weights=np.zeros_like)


def _segment_problem(entries):
    """One graph of 17 nodes.  The first tile (rows 0 .. 15) receives `entries` edges in all, row i the i-th share of them,
    from senders spread over all 17 nodes (parallel edges included); node 16, the second tile's only live row, has a self loop."""
    n = 17
    s, r = [], []
    for i in range(16):
        for q in range(entries // 16 + (i < entries % 16)):
            s.append((7 * i + 3 * q + 1) % n), r.append(i)
    assert len(s) == entries
    s.append(16), r.append(16)
    rng = np.random.default_rng(1000 + entries)
    return dict(hp=_hp(D, L, K, "mean", "leaky_relu"), nn=np.array([n], np.int32), ne=np.array([len(s)], np.int32),
                s=np.asarray(s, np.int32), r=np.asarray(r, np.int32), n=n, d=D,
                x=rng.standard_normal((n, D)).astype(np.float32), zs=rng.standard_normal((n, D)).astype(np.float32),
                p=O.make_grevnet_params(D + K + entries, D // 2, L, K, T, final_scale=0.3))


@pytest.mark.parametrize("entries", [0, 1, 511, 512, 513, 2048, 2049])
def test_col_segment_lengths_in_front_of_the_bias_block(force_shape, entries):
    _three_way(_segment_problem(entries), LAYOUTS["contiguous"], force_shape)


@pytest.mark.parametrize("gname,net", [("n47_three_graphs", "mean_leaky"), ("isolated_and_deg9to17", "sum_relu")])
def test_two_runs_with_nan_refilled_buffers_agree(force_shape, gname, net):
    pr = _with_distinct_biases(_problem(gname, *NETS[net]))
    first, second, generic = _run(pr, LAYOUTS["contiguous"], force_shape, (AUTO, AUTO, GENERIC))
    _assert_same(first, second, "two runs of automatic dispatch, NaN-filled workspace and destination in between")
    _assert_same(first, generic, "automatic dispatch vs force_shape = 12")
