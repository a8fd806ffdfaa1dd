"""The message-passing backward walk without batch norm (gnf_grevnet_backward_f32, csrc/gnf_train.hip) on directed, skewed
batches, one pytest id per (case, route).  The cases (tests/backward_routes.py; their premises are held by
tests/test_backward_routes_cpu.py) are the smallest shapes at which each branch of the walk exists:

  n1, noedges       one node with self loops only; E = 0 for the whole batch
  n17, n33          a tile boundary inside a graph, isolated rows, a last tile with one live row; three tiles whose
                    by-sender CSR differs from the by-receiver one across tiles
  star_in, star_out tile 0's by-receiver / by-sender edge slice is longer than kBwdColCap = 2048 ints, the other one short:
                    the un-staged column reads of tile_aggregate (recomputing tile kernel) / of the fold
  n3072 | n3073     merged_walk_ok: (n + 15) / 16 <= kMergedMaxTiles = 192.  At 3072 the call takes half_merged (one launch per
                    half-step: tile kernel + the previous half-step's dW + the reduce before it, the scatter folded into the
                    next prologue, the pipeline drained at the end), at 3073 half_streams with launch_half_bwd_fused_stashed.
                    The library exposes nothing that tells the two apart: both sides are run and held to the oracle.
  n4096 | n4097     mlp_stash_supported / fused_stash_shape: sixteen-row tiles <= the CU count (256).  At 4097 no stash is
                    offered and fused_bwd_launch_shape goes to 32-row workgroups.
Hyper-parameters vary over the cases so that sum / mean, agg / concat, epsilon 0 / 0.5 / 1, relu / leaky_relu, weight
sharing, K = 1 / 3, odd H (scalar k_aggregate_bwd) / H = 4 (vec4), T = 1 (drain with one pending plan) / 2 (four half-steps
on three operand sets) / 3 each appear at least twice.

Routes (backward_routes.ROUTES): 1 default; 2 recompute (tr.stash_mlp_rows = False); 3 layered (net.fused = False: layered
forward, generic backward - with the layered mode of the stash at K >= 2, layered_stash_mode); 4 bwd_generic (option
bwd_generic = 1: fused forward, generic backward, no stash); 5 dw_grouped (option dw_grouped = 1: the tile kernel without the
merged launch - k_aggregate_bwd in a launch of its own, the dW GEMMs on the auxiliary stream); 6 dw_grouped_serial (5 with
tr.overlap_weight_grads = False).

Every (case, route): z, loss and log-det by check_forward_terms' rules, the reconstruction by check_reconstruction, every
gradient tensor against O.loss_and_grads in float64 under two tiers, a second loss_and_grads on the same trainer bitwise
equal to the first (overwritten, not accumulated), and the stash evidence: tr._mlp_stash and gnf_mlp_stash_bytes > 0 exactly
for n <= 4096 on routes 1, 5, 6; none on routes 2 and 4; on route 3 exactly at K >= 2.
  project tier: 3e-4 max|g| + 1e-5 + 1e-6 gmax per tensor, widened to 4 x the float32 oracle's deviation of that tensor;
  tight tier:   SLACK x the float32 oracle's deviation of that tensor + 1e-6 gmax, never looser than the project tier.
Seeds: the first in range(16) whose kink band (|pre-activation| < 2e-5 in float64) is empty for n1 .. n33 and holds at most
16 hidden units for the others; a tensor that misses is compared once more against float64 autograd with the device's sides
for THOSE units (batch_norm_routes' fit).  On the unmodified library no case needed the fit.

test_routes_agree, per case.  Bitwise equal by construction, asserted with torch.equal:
  5 = 6 at every n        the same launches with the same arguments; only the stream of the dW launches differs
  1 = 5 at 3072 < n <= 4096  neither is merged, both run launch_half_bwd_fused_stashed + k_aggregate_bwd, and dw_policy
                          gives both the grouped dW kernel (more than 192 backward tiles: max_units = 0, as under the option)
  1 = 2 at n > 4096       no stash is offered, so "default" IS the recomputing walk
Measured bitwise equal as well, but not promised by the code and so not asserted: 2 = 4 wherever neither is merged (the
generic GEMM path and the tile kernel produce the same dW operands bit for bit at these widths), 1 = 5 at n = 1, 5 and 4097.
Every other route is held to the default route by the tight bound on the difference of their residuals (gradient minus
the float64 gradient it was held to).

Measured on an MI355X, float32 oracle on that machine's CPU: worst err / dev32 over the tensors of a (case, route), where
err is the device's and dev32 the float32 oracle's max deviation from the float64 gradient of that tensor (tensors the
float32 oracle gets exactly, dev32 = 0, are left out while the device is within 1e-6 gmax of them); 70 tests, 3.1 s
  case       default  recompute  layered  bwd_generic  dw_grouped  dw_grouped_serial
  n1           3.04      3.04      3.04       3.04        3.04          3.04
  noedges      3.45      2.43      2.22       2.43        3.45          3.45
  n17          2.97      3.81      5.66       3.81        3.54          3.54
  n33          5.83      5.83      5.83       5.45        5.83          5.83
  star_in     10.09     10.09      6.40       9.24        9.24          9.24
  star_out     2.25      2.25      3.98       5.23        5.23          5.23
  n3072        5.92      5.92      5.92       7.07        7.07          7.07
  n3073        7.01      8.29      6.16       8.29        7.01          7.01
  n4096        2.00      1.81      1.58       1.81        2.00          2.00
  n4097        5.11      5.11      5.11       5.11        5.11          5.11
  worst       10.09     10.09      6.40       9.24        9.24          9.24
No route stands out on any case (the worst, star_in s[0][0].b1: device 1.77e-7 of max|g|, float32 oracle 1.75e-8 - a tensor
the float32 oracle happens to get almost exactly).  SLACK = 4 x 10.09 = 40.4.  Over the 1584 (case, route, tensor) figures the device is
within 1.3e-8 .. 1.6e-6 of a tensor's max (median 1.5e-7), the float32 oracle within 1.1e-8 .. 2.3e-6 (median 1.3e-7; never
exactly 0): SLACK x dev32 is 5e-6 of a tensor's max at the median and 3e-5 at the ninth decile, where the project tier
allows 3e-4.

What the tests found: no defect in the library.  Two statements of the plan did not hold and were corrected in the tests:
"every case has csr != csr_t" cannot hold for n1 and noedges (held to equality there instead), and the first mutation
below does NOT pass the earlier suite.

That the tests bite: three numeric-only mutations (all reads stay in bounds), each built in a scratch copy and run once
  a. the fold (gnf_fused_bwd_dev.h) reads a.col in place of a.col_t: fails n17, n33, star_in, star_out, n3072 on routes
     1 and 2 (the merged walk: the only one with a fold) and test_routes_agree of those five cases; n1, noedges (col == col_t)
     and n3073 .. n4097 (not merged) pass.  Of the 1418 earlier GPU tests exactly two fail as well,
     test_isolated_nodes_and_directed_edges and test_randomised_parity_sweep (case 3, one directed graph of 14 nodes): a
     five-node batch with T = 2 does run the fold, so the earlier suite was not blind to this one.
  b. the un-staged branch of the fold's colat returns a.col_t[e - 1] for e > beg: fails star_out on routes 1 and 2 and
     test_routes_agree[star_out], through the side fit's own guard ("kink fit is not a set of sides": the difference is no
     combination of relu sides); everything else passes, the earlier directed test and the sweep included.
  c. k_aggregate_bwd without the invdeg weight: fails the mean cases wherever the scatter has its own launch - n1, n33,
     star_in, n3072 on routes 3 - 6, n4096 on all six - and their test_routes_agree; the sum cases pass.  (n1 .. n3072 on
     routes 1 and 2 pass: there only the walk's last half-step runs k_aggregate_bwd, into dL/dx, which no weight gradient
     reads.)  Of the earlier tests run against it, test_randomised_parity_sweep fails."""
import numpy as np
import pytest
import torch

import backward_routes as R
import batch_norm_routes as B

pytestmark = pytest.mark.gpu

SLACK = 40.4       # 4 x 10.09, the largest err / dev32 measured (table above)
ROUTES = list(R.ROUTES)
TILE_ROUTES = ("default", "dw_grouped", "dw_grouped_serial")      # the stash is offered: routes 1, 5 and 6


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


_GRADED = {}


def _grade(c, route):
    """One (case, route) against the case's shared reference, once: (report, largest needed slack, the float64 gradient the
    run was held to - the oracle's own, or the one with the device's sides for the units inside the kink band)."""
    if (c, route) in _GRADED:
        return _GRADED[c, route]
    ref, pr = R.reference(c), R.problem(c)
    got = R.device_run(c, route)
    n = pr["n"]
    rep = R.Report(f"{c.name} {route}")
    B.check_forward_terms(rep, got, ref, n)
    B.check_reconstruction(rep, got, pr["x"])
    worst, want = R.check_grads(rep, got, ref, c, SLACK)
    again = float((got["flat"] - got["flat_again"]).abs().max()) if got["flat"].numel() else 0.0
    print(f"[bwd-routes] {rep.title}: n {n} seed {pr['seed']} worst ratio {worst:.2f}; second call differs by {again:.3e}; "
          f"stash {got['stash']} ({got['stash_bytes']} bytes offered)")
    if not torch.equal(got["flat"], got["flat_again"]):
        rep.bad.append(f"a second loss_and_grads on the same trainer changed the gradient by {again:.3e}")
    # route evidence: what the library exposes about the MLP-row stash
    if route in TILE_ROUTES:
        want_stash = n <= 4096
        if got["stash"] != want_stash or (got["stash_bytes"] > 0) != want_stash:
            rep.bad.append(f"stash {got['stash']} / {got['stash_bytes']} bytes offered, expected {'one' if want_stash else 'none'} at n = {n}")
    elif route == "recompute":
        if got["stash"]:
            rep.bad.append("stash_mlp_rows = False, yet the trainer holds a stash")
    elif route == "bwd_generic":
        if got["stash"] or got["stash_bytes"]:
            rep.bad.append(f"bwd_generic = 1, yet a stash was offered ({got['stash_bytes']} bytes)")
    else:
        if got["stash"] != (c.k >= 2) or (got["stash_bytes"] > 0) != (c.k >= 2):
            rep.bad.append(f"layered: stash {got['stash']} / {got['stash_bytes']} bytes offered at K = {c.k}")
    _GRADED[c, route] = (rep, worst, want)
    return _GRADED[c, route]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_route_against_the_oracle(c, route):
    """Forward terms, reconstruction, both gradient tiers, the repeated call and the stash evidence of one (case, route)."""
    rep, _, _ = _grade(c, route)
    rep.finish()


def _bitwise_pairs(n):
    """The pairs of routes the dispatch code makes run the same launches on the same operands (module docstring)."""
    pairs = [("dw_grouped", "dw_grouped_serial")]
    if 3072 < n <= 4096:
        pairs.append(("default", "dw_grouped"))
    if n > 4096:
        pairs.append(("default", "recompute"))
    return pairs


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_routes_agree(c):
    """Across the six routes of one case: torch.equal for the pairs of _bitwise_pairs, every route against the default
    one to the tight bound (on the residuals, so that a relu side taken differently by two routes is not held against
    either).  Every pair's difference is printed."""
    ref, n = R.reference(c), R.problem(c)["n"]
    runs = {route: R.device_run(c, route) for route in ROUTES}
    held = {route: _grade(c, route)[2] for route in ROUTES}
    bad = []
    for a, b in [(x, y) for i, x in enumerate(ROUTES) for y in ROUTES[i + 1:]]:
        same = torch.equal(runs[a]["flat"], runs[b]["flat"])
        diff = float((runs[a]["flat"] - runs[b]["flat"]).abs().max()) if runs[a]["flat"].numel() else 0.0
        print(f"[bwd-routes] {c.name} {a} vs {b}: {'bitwise equal' if same else f'max difference {diff:.3e}'}")
        if (a, b) in _bitwise_pairs(n) and not same:
            bad.append(f"{a} vs {b}: not bitwise equal (max difference {diff:.3e})")
    gmax = max(float(np.abs(g).max()) for _, g in ref["grads"])
    for b in ROUTES[1:]:
        for (nm, ga), (_, wa), (_, gb), (_, wb), (_, g64) in zip(runs["default"]["grads"], held["default"], runs[b]["grads"],
                                                                 held[b], ref["grads"]):
            top, dev = float(np.abs(g64).max()), ref["dev"]["grads"][nm]
            err = float(np.abs((ga - wa) - (gb - wb)).max())
            tight = min(SLACK * dev + 1e-6 * gmax, max(3e-4 * top + 1e-5 + 1e-6 * gmax, 4.0 * dev))
            if not err <= tight:
                bad.append(f"default vs {b}, {nm}: {err:.3e} > {tight:.3e}")
    assert not bad, c.name + "\n" + "\n".join(bad)
