"""What tests/test_backward_routes_gpu.py rests on, checked where it can be checked without a device: every case has a
seed under the kink-band rule, inputs the oracle can take and a well-conditioned reversible round trip; the topologies put
the tiles where the case's name says (node counts on both sides of each route limit, the long by-receiver / by-sender slice
of tile 0 past the backward tile kernel's 2048-int column buffer, kBwdColCap in csrc/gnf_fused_bwd_dev.h), and no case's by-sender CSR
equals its by-receiver CSR - the property every earlier message-passing gradient test lacked."""
import numpy as np
import pytest

import backward_routes as R

CASES = pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
COL_CAP = 2048      # kBwdColCap


@CASES
def test_case_has_a_seed_and_the_oracle_takes_it(c):
    picked = R.pick_seed(c)
    assert picked is not None, f"no seed in range(16) leaves at most {c.band} hidden units in the kink band: change the case"
    seed, pr, kink = picked
    ref = R.reference(c)
    rt = R.round_trip32(pr, c.t)
    rel = max(ref["dev"]["grads"][nm] / max(float(np.abs(b).max()), 1e-30) for nm, b in ref["grads"] if np.abs(b).max() > 0)
    print(f"{c.name}: seed {seed}, n {pr['n']}, E {len(pr['s'])}, |z|max {np.abs(ref['z']).max():.2f}, {len(kink['units'])} of "
          f"{kink['total']} hidden units within {kink['tol']:.1e} of a kink, float32 round trip {rt:.1e}, float32 gradients "
          f"within {rel:.1e} of each tensor's max")
    assert len(kink["units"]) <= c.band
    assert np.isfinite(ref["z"]).all() and np.abs(ref["z"]).max() < 50.0
    assert all(np.isfinite(b).all() for _, b in ref["grads"]) and np.isfinite(ref["loss"])
    assert max(float(np.abs(b).max()) for _, b in ref["grads"]) > 1e-3          # a gradient worth comparing
    assert rt < 1e-5
    assert pr["x"].dtype == np.float32 and pr["x"].shape == (pr["n"], c.d)
    assert int(pr["nn"].sum()) == pr["n"] and int(pr["ne"].sum()) == len(pr["s"]) == len(pr["r"])
    # edges stay inside their graph
    first = np.repeat(np.cumsum(pr["nn"]) - pr["nn"], pr["ne"])
    last = np.repeat(np.cumsum(pr["nn"]), pr["ne"])
    assert ((pr["s"] >= first) & (pr["s"] < last) & (pr["r"] >= first) & (pr["r"] < last)).all()


def test_hyper_parameters_cover_every_branch_twice():
    """agg, combine, epsilon, activation (where a hidden layer exists), weight sharing, K = 1 and 3, the scalar (odd H) and
    the vec4 (H % 4 == 0) instance of k_aggregate_bwd, T = 1, 2, 3: each at least twice over the cases."""
    cs = R.CASES
    count = lambda pred: sum(1 for c in cs if pred(c))      # noqa: E731
    for agg in ("sum", "mean"):
        assert count(lambda c: c.agg == agg) >= 2
    for combine in ("agg", "concat"):
        assert count(lambda c: c.combine == combine) >= 2
    for eps in (0.0, 0.5, 1.0):
        assert count(lambda c: c.eps == eps) >= 2
    for act in ("relu", "leaky_relu"):
        assert count(lambda c: c.act == act and c.k > 1) >= 2
    assert count(lambda c: c.ws and c.t > 1) >= 2
    assert count(lambda c: c.k == 1) >= 2 and count(lambda c: c.k == 3) >= 2
    assert count(lambda c: (c.d // 2) % 2 == 1) >= 2 and count(lambda c: (c.d // 2) % 4 == 0) >= 2
    for t in (1, 2, 3):
        assert count(lambda c: c.t == t) >= 2
    assert all(4 <= c.d <= 10 and 16 <= c.latent <= 24 and c.k <= 3 for c in cs)
    assert R.BY_NAME["star_in"].agg == "mean"
    assert all(R.final_scale(c) == 0.05 for c in cs if c.agg == "sum")


@CASES
def test_by_sender_csr_differs_from_by_receiver_csr(c):
    """Two cases cannot differ and are held to that instead: noedges (E = 0: both CSRs are empty) and n1 (one node: every
    edge is a self loop, so both are rowptr [0, E], col all zero)."""
    (rp, col), (rp_t, col_t) = R.csr_pair(R.problem(c))
    assert len(col) == len(col_t) == len(R.problem(c)["s"])
    if c.name in ("noedges", "n1"):
        assert np.array_equal(rp, rp_t) and np.array_equal(col, col_t) and not col.any()
        assert (len(col) == 0) == (c.name == "noedges")
        return
    assert not np.array_equal(rp, rp_t) and not np.array_equal(col, col_t)


@pytest.mark.parametrize("name", ["star_in", "star_out"])
def test_star_puts_one_slice_of_tile_0_past_the_column_buffer(name):
    """Tile 0 = rows 0..15.  star_in: its by-receiver slice (tile_aggregate of the recomputing kernel) is longer than
    kBwdColCap ints and its by-sender slice (the fold) shorter; star_out: the other way round.  Every other tile of either
    CSR stays under the cap, so exactly one un-staged read path runs per case."""
    c = R.BY_NAME[name]
    (rp, _), (rp_t, _) = R.csr_pair(R.problem(c))
    long_rp, short_rp = (rp, rp_t) if name == "star_in" else (rp_t, rp)
    assert long_rp[16] - long_rp[0] > COL_CAP
    assert short_rp[16] - short_rp[0] < COL_CAP
    for q in (rp, rp_t):
        tiles = [q[min(i + 16, len(q) - 1)] - q[i] for i in range(16, len(q) - 1, 16)]
        assert max(tiles) < COL_CAP


@pytest.mark.parametrize("name", ["n3072", "n3073", "n4096", "n4097"])
def test_route_limits_are_bracketed(name):
    """(n + 15) / 16 <= kMergedMaxTiles = 192 (merged_walk_ok, gnf_train.hip): 3072 | 3073; sixteen-row tiles <= the CU
    count, 256 (mlp_stash_supported, fused_stash_shape; fused_bwd_launch_shape goes to 32-row workgroups past it): 4096 | 4097."""
    n = R.problem(R.BY_NAME[name])["n"]
    assert n == int(name[1:])
    assert ((n + 15) // 16 <= 192) == (name == "n3072")
    assert ((n + 15) // 16 <= 256) == (name in ("n3072", "n3073", "n4096"))
