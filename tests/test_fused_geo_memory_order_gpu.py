"""The memory order of the compile-time-geometry half-step kernel (k_half_fused_geo, gnf_fused.hip): the rowptr slice, the
thread's own x_cond[r, f] and its old x_upd_src[r, f] are requested at kernel entry; the first 512 entries of a tile's col
segment go through a register in front of the weight prefetch, the entries behind them through the staging loop, and a
segment above the LDS slice (2 048 entries) stays in global memory; sum(s) and sum(z^2) leave through one reduction pass.
Only when loads are issued and waited for differs from the generic k_half_fused<1, 2>, so every case asserts torch.equal
between automatic dispatch and gnf_set_option("force_shape", 12) on z, on [logdet, sum z^2] and on the inverse's x, then the
float64 oracle bounds of test_fused_geo_gpu.py (whose runner, checks and fixtures are used as they are).

Every case is D = 64, L = 256, K = 5, T = 2: four half-steps - the out-of-place first one (x_upd_src is the source buffer,
x_upd and cond_copy the destination), the in-place ones, and the two that write sq_partials.

Shapes:
  col segment of a tile: 0, 1, 511, 512, 513, 2 048, 2 049 entries in tile 0 of a 48-node graph - repeated edges onto its
      sixteen rows, listed in shuffled order - beside a tile of sixteen degree-0 rows and a tile holding a ring.  Segments of
      511 and more use `mean` (a sum over 128 neighbours per row would overflow exp(s)); the oracle's z is checked to be
      finite and below 1e4 for every case when the problem is built.
  row count: 1, 16, 17 (the r < n_nodes guard of the two hoisted own-row loads; guard bands behind the rows are checked).
  layout: a row stride above D on a base 12 bytes off 16-byte alignment, on the 513-entry segment and on 17 rows."""
from functools import lru_cache

import numpy as np
import pytest

from oracle import gnf_oracle as O
from test_fused_geo_gpu import (D, K, L, LAYOUTS, NETS, T, _assert_equal_and_oracle, _batch_of, _hp,  # noqa: F401
                                _require_gpu_and_native_lib, _rings, _ring, _run_both, force_shape)

pytestmark = pytest.mark.gpu

N_SEG = 48          # three 16-row tiles: the long segment | sixteen degree-0 rows | a ring
SEG_LENGTHS = [0, 1, 511, 512, 513, 2048, 2049]


def _segment_graph(seg_len):
    """One graph of 48 nodes.  Rows 0 .. 15 (tile 0) receive `seg_len` edges in all, dealt round-robin over the rows, senders
    walking over all 48 nodes (so edges repeat); rows 16 .. 31 have no incoming edge; rows 32 .. 47 form a ring with self
    loops.  The edge list is shuffled: a receiver's edges are not contiguous in the input."""
    s = [(7 * e + 3) % N_SEG for e in range(seg_len)]
    r = [e % 16 for e in range(seg_len)]
    rs, rr = _ring(16, 32)
    s, r = np.asarray(s + rs, np.int32), np.asarray(r + rr, np.int32)
    order = np.random.default_rng(seg_len).permutation(len(s))
    return _batch_of([(N_SEG, s[order], r[order])])


GRAPHS = {f"seg{n}": (lambda n=n: _segment_graph(n)) for n in SEG_LENGTHS}
GRAPHS.update({"n1": lambda: _rings([1]), "n16": lambda: _rings([16]), "n17": lambda: _rings([17])})


@lru_cache(maxsize=None)
def _problem(gname, agg, act):
    """Batch, inputs, parameters and the float64 oracle's results: computed once per (graph, net), shared by the layouts."""
    nn, ne, s, r = GRAPHS[gname]()
    n = int(nn.sum())
    hp = _hp(D, L, K, agg, act)
    rng = np.random.default_rng(sum(map(ord, gname + agg + act)))
    x = rng.standard_normal((n, D)).astype(np.float32)
    zs = rng.standard_normal((n, D)).astype(np.float32)
    p = O.make_grevnet_params(D + K, D // 2, L, K, T, final_scale=0.3 if agg == "mean" else 0.1)
    o = O.Fp64Dense(s, r, n, agg=agg, activation=act)
    ref, xg = o.log_prob(x, p, T), o.g(zs, p, T)
    seg0 = int(np.count_nonzero(np.asarray(r) < 16))
    assert agg == "mean" or seg0 < 511, "long segments use mean"
    for name, v in (("z", ref["z"]), ("g(zs)", xg)):   # (checked on the CPU before anything runs on the device)
        assert np.isfinite(v).all() and np.abs(v).max() < 1e4, f"{gname}/{agg}/{act}: the oracle's {name} is out of range"
    return dict(hp=hp, nn=nn, ne=ne, s=s, r=r, n=n, d=D, x=x, zs=zs, p=p, ref=ref, xg=xg)


SEG_CASES = [(0, "mean_leaky"), (0, "sum_relu"), (1, "sum_leaky"), (1, "mean_relu"), (511, "mean_leaky"), (512, "mean_relu"),
             (513, "mean_leaky"), (2048, "mean_relu"), (2049, "mean_leaky")]


@pytest.mark.parametrize("seg_len,net", SEG_CASES)
def test_col_segment_lengths(force_shape, seg_len, net):
    pr = _problem(f"seg{seg_len}", *NETS[net])
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS["contiguous"], force_shape))


@pytest.mark.parametrize("gname,net", [("n1", "sum_relu"), ("n16", "mean_leaky"), ("n17", "sum_leaky"), ("n17", "mean_relu")])
def test_row_counts(force_shape, gname, net):
    pr = _problem(gname, *NETS[net])
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS["contiguous"], force_shape))


@pytest.mark.parametrize("gname,net", [("seg513", "mean_leaky"), ("n17", "sum_leaky")])
def test_strided_misaligned_rows(force_shape, gname, net):
    pr = _problem(gname, *NETS[net])
    _assert_equal_and_oracle(pr, _run_both(pr, LAYOUTS["ldD+3_c3"], force_shape))
