"""The wide-layer kernels (csrc/gnf_linear_big.hip: k_linear_big, its transposed and its thin-last-layer forms, and
k_linear_short) against the generic tile, with a proof of the route.

Nets too wide for the LDS-resident kernels run layer by layer, and two hand-scheduled kernels carry their wide layers where
launch_linear_big_impl / launch_linear_short accept the call; where they answer "not my case" the generic tile runs without
a word.  net.fused = False hides the packed weight copies, so the same net then runs on the generic tile alone: the A/B of
this module.  The wide kernels read the packed fragment copy, the generic tile the raw W - perturbing one and not the other
proves which kernel ran (section 1), and everything else stands on that.

What is compared, and how
  * Route proof: Wp_j (forward: k_linear_short, k_linear_big, the thin-last-layer epilogue) or WpT_j (dX) of one half-step's
    nets times 2 in place.  z must change; with the whole route bitwise it must equal the generic tile's z on 2 W_j; dW_0, db_0
    must come out exactly 2 x with every later layer's gradient untouched; fused = False must not notice; 7 inputs (no whole
    float4) must stay on the generic tile.
  * Bit equality with the generic tile - z, the log-det / sum z^2 pair, the inverse, the training forward, the reconstruction
    and every gradient tensor in both stash modes, no element left out - HOLDS on the MI355X for
      k_linear_big forward        every row deal (MW = 2, 3, 4, the trailing 1-tile workgroup, a ragged last tile, two rounds),
                                  widths 512, 528 (33 k-groups), 1030 (no multiple of 4), 1040, 1280, relu and leaky_relu,
                                  a last layer without activation, 75 k-groups (four chunks and an odd rest);
      k_linear_big transposed     the same deals and widths, masked (relu: plenty of exact zeros in aux) and with aux == NULL
                                  at 256 (one column block), 300 and 1200 output columns;
      k_linear_short              all four instances: 1, 7 (cut to one float4), 8, 9, 11, 11 (cut), 13 k-groups into 1296 columns
                                  (the last column block of either instance has one live tile) and 1280, wg_rem > 0, two rounds.
    The headers of both kernels in csrc/gnf_linear_big.hip say so.
  * NOT bitwise, by design: the thin last layer out of k_linear_big's accumulators (column-block slabs added in another
    order), and a net the LDS-resident forward kernel holds.  Both routes are compared with the float64 oracle instead.

What the route proof found
  fused_fits_lds looks at the WIDEST layer of a net, not at "wide or not": K = 3 nets with hidden widths up to about 1130
  (512, 528, 1030, 1040 of this module's list) run their forward and inverse passes in k_half_fused unless the input or
  output is wider, and only the backward walk (recompute and dX) reaches the wide kernels.  So these widths are tested
  twice: as D = 2400 nets (H = 1200 keeps the flow layered, and then ALL THREE layers are k_linear_big's in both directions),
  bit for bit; and at latent 1040 by the exact-2x proof of the backward walk plus the oracle comparison of z.  For the same reason
  k_linear_short is taken at hidden widths 1296 / 1280 in K = 2 nets in -> L -> in, where it is the only difference between
  the routes; its first-layer role in front of k_linear_big is what the D = 288 cases run.
  The workspace's leading dimension follows the hidden width (hidden_max): at 1030 ldx, ldy and ldaux are off 16-byte
  alignment, so fetch, the epilogue store and the mask read go element by element on EVERY float4, not only the last;
  launch_linear_short refuses such a net (O & 3, ldy & 3) and its first layer stays on the generic tile.
  dX of a first layer (aux == NULL) has in0 output columns: at in0 = 256 that is two panels, and the launcher takes it from
  512 row tiles on.

Every precondition a case is named after (the deal, the instance, which kernels can hold the net) is asserted from
tests/wide_linear_cases.py's restatements before the case runs, with the chip's own CU count: on another chip the case
fails instead of testing something else.  The restatements are never an expected value.

Measured on the MI355X (256 CUs); no bound was changed.  Bitwise cases: 0 differing elements in every tensor.  Worst ratio
(device deviation / bound) of the oracle cases, wide route | generic route:
  D130 L1280 (H = 65)     z 0.109 | 0.115   round trip 0.098 | 0.098   worst gradient tensor 0.216 | 0.216
  D200 L1280 (H = 100)    z 0.116 | 0.116   round trip 0.098 | 0.098   worst gradient tensor 0.000 | 0.002
  D200 L1296 (H = 100)    z 0.116 | 0.114   round trip 0.098 | 0.098   worst gradient tensor 0.000 | 0.000
  D300 L1040 (LDS fwd)    z 0.183 | 0.122   round trip 0.098 | 0.098   (gradients: see the test's docstring)
Teeth (local builds, not committed): with k_linear_big's mask comparison `> 0.f` turned into `>= 0.f` every relu case of the
bitwise gradient tests fails (32 of 57 tensors differ) and the oracle cases read 700 - 950 x their bound; with
launch_linear_short returning 1 unconditionally the three layer-0 route proofs fail while every parity test still passes.
"""
import numpy as np
import pytest
import torch

from helpers import graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O
from test_fullsize_gpu import FLOOR, SLACK, _conditioning

import wide_linear_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_GRAPHS = {}


def _graph(n, d, seed=7):
    """(device graph, (n_node, n_edge, senders, receivers), x) of exactly n nodes; built once per (n, d)"""
    if (n, d, seed) not in _GRAPHS:
        nn, ne, s, r = W.ring_batch(n)
        assert int(nn.sum()) == n
        x = W.features(n, d, seed)
        _GRAPHS.clear()                      # (one batch at a time: the largest are 8 k rows x 512 and 4 k rows x 2400 columns)
        _GRAPHS[(n, d, seed)] = (graph_from_arrays(nn, ne, s, r, x, DEV), (nn, ne, s, r), x)
    return _GRAPHS[(n, d, seed)]


def _net(hp, p, fused):
    net = make_product_grevnet(hp, p)
    net.fused = fused
    return net


def _forward(net, graph):
    zg, _ = net(graph, inverse=True)
    torch.cuda.synchronize()
    return zg.nodes.clone(), net.last_sums.clone()


def _packed(net):
    return net._cache[2][3]                  # the flow's packed copies: all s-nets (half * T + step), then all t-nets


def _scale_region(net, dims, kind, j, half, factor=2.0):
    """multiply Wp_j ("w") or WpT_j ("wt") of the s- and the t-net of one half-step in place (powers of 2: exact)"""
    buf = _packed(net)
    per_net = W.packed_floats(dims)
    assert buf.numel() == 4 * per_net, (buf.numel(), per_net)      # T = 1: two s-nets, two t-nets
    off, ln = W.packed_region(dims, kind, j)
    for k in ("s", "t"):
        base = W.net_index(k, half) * per_net + off
        buf[base:base + ln].mul_(factor)
    torch.cuda.synchronize()


def _grad_tensors(tr, hp):
    """[(name, flat slice of tr.grad)] in the arena's order: s-nets, then t-nets, (W_j, b_j) per layer"""
    out, off = [], 0
    dims = W.net_dims(hp["D"], hp["latent"], hp["K"], hp["combine"])
    for kind in ("s", "t"):
        for half in range(2):
            for j in range(hp["K"]):
                for name, cnt in ((f"{kind}[{half}].W{j}", dims[j] * dims[j + 1]), (f"{kind}[{half}].b{j}", dims[j + 1])):
                    out.append((name, slice(off, off + cnt)))
                    off += cnt
    assert off == tr.grad.numel()
    return out


def _train(hp, p, graph, fused, stash):
    from gnf_amd.train import GRevNetTrainer
    net = _net(hp, p, fused)
    tr = GRevNetTrainer(net)
    tr.stash_mlp_rows = stash
    out = tr.loss_and_grads(graph)
    torch.cuda.synchronize()
    return tr, out


def _everything(hp, p, graph, fused, z_for_inverse=None):
    """forward, inverse and both training walks of one route -> {name: device tensor}"""
    net = _net(hp, p, fused)
    res = {}
    res["z"], res["sums"] = _forward(net, graph)
    zin = res["z"] if z_for_inverse is None else z_for_inverse
    res["inverse"] = net(graph.replace(nodes=zin), inverse=False).nodes.clone()
    for stash in (True, False):
        tag = "stash" if stash else "recompute"
        tr, out = _train(hp, p, graph, fused, stash)
        res[f"train_z[{tag}]"] = out["z_graph"].nodes.clone()
        res[f"train_sums[{tag}]"] = out["sums"].clone()
        res[f"reconstruction[{tag}]"] = out["reconstruction"].clone()
        for name, sl in _grad_tensors(tr, hp):
            res[f"d{name}[{tag}]"] = tr.grad[sl].clone()
    torch.cuda.synchronize()
    return res


def _assert_same_bits(label, got, want):
    """every tensor of `got` equals its partner bit for bit; the differing ones are printed before the assertion"""
    bad = []
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape and bool(torch.isfinite(b).all()), name
        if not torch.equal(a, b):
            diff = (a.double() - b.double()).abs()
            bad.append((name, int((a != b).sum()), a.numel(), float(diff.max()), float(b.double().abs().max())))
    print(f"[wide] {label}: {len(want) - len(bad)} of {len(want)} tensors bit-identical")
    for name, cnt, tot, dmax, ref in bad:
        print(f"[wide]   {label}: {name}: {cnt} of {tot} elements differ, max |diff| {dmax:.3e} (max |ref| {ref:.3e})")
    assert not bad, f"{label}: {[b[0] for b in bad]}"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Route proof
# ---------------------------------------------------------------------------------------------------------------------------
ROUTE_N = 1664
# dX of layer 0 has in0 output columns: one column block (two panels) at in0 = 256, two at 300 - the launcher wants 1024 row-tile
# units on 256 CUs, i.e. 512 and 256 row tiles (at either size the generic tile has over 192 tiles and does not split K)
NO_MASK_N = {512: 8180, 300: 4090}


def _route_setup(d, latent, combine="agg", k=3, n=ROUTE_N, act="relu", lds_forward=False):
    hp = W.make_hp(d, latent, k=k, combine=combine, act=act)
    dims = W.net_dims(d, latent, k, combine)
    assert W.fused_fwd_fits(dims) == lds_forward and not W.fused_bwd_fits(dims), "this net would run the LDS-resident kernels"
    p = W.make_params(hp, 61)
    graph = _graph(n, d)[0]
    return hp, dims, p, graph


@pytest.mark.parametrize("j,owner", [(0, "k_linear_short<7,4>"), (1, "k_linear_big"), (2, "k_linear_big's thin-last-layer epilogue")],
                         ids=["layer0_short", "layer1_big", "layer2_thin_last"])
@pytest.mark.parametrize("half", [0, 1], ids=["half0", "half1"])
def test_route_forward_reads_the_packed_copy_of_every_layer(j, owner, half):
    """D = 200, latent 1280, K = 3 on 1664 rows: doubling Wp_j of one half-step's nets (raw W_j untouched) changes z - the
    kernel that ran layer j read the packed copy, and only the wide kernels do in the layered path; with fused = False the
    same perturbation of that net's buffer changes nothing."""
    hp, dims, p, graph = _route_setup(200, 1280)
    assert W.short_deal(ROUTE_N, dims[0], dims[1], _cus()) and W.big_deal(ROUTE_N, dims[2], _cus()) and W.fused_last(dims, 2)
    net = _net(hp, p, True)
    z0, s0 = _forward(net, graph)
    z0b, s0b = _forward(net, graph)
    assert torch.equal(z0, z0b) and torch.equal(s0, s0b), "two calls differ: nothing can be proved by a change"
    _scale_region(net, dims, "w", j, half)
    z1, _ = _forward(net, graph)
    changed = int((z1 != z0).sum())
    print(f"[wide] route forward: layer {j} ({owner}), half {half}: {changed} of {z0.numel()} elements of z follow Wp_{j}")
    assert changed > 0, f"layer {j}: z does not depend on the packed copy - {owner} did not run"
    assert bool(torch.isfinite(z1).all())
    net.repack()
    z2, _ = _forward(net, graph)
    assert torch.equal(z2, z0), "the re-packed net does not give the first call's bits"
    # the generic route never reads the buffer
    gen = _net(hp, p, False)
    g0, _ = _forward(gen, graph)
    _scale_region(gen, dims, "w", j, half)
    g1, _ = _forward(gen, graph)
    assert torch.equal(g0, g1), "fused = False read the packed buffer"


@pytest.mark.parametrize("j", [0, 1])
def test_route_forward_equals_the_generic_tile_on_doubled_weights(j):
    """D = 288 (H = 144: a last layer the wide kernel does not take along; 144 inputs: k_linear_short<11,2>), latent 1280:
    z of the net whose Wp_j was doubled in place equals, bit for bit, z of a fused = False net whose raw W_j was doubled
    (a power of two: the comparison adds no tolerance)."""
    hp, dims, p, graph = _route_setup(288, 1280)
    assert W.short_deal(ROUTE_N, dims[0], dims[1], _cus())["instance"] == "11x2" and not W.fused_last(dims, 2)
    net = _net(hp, p, True)
    z0, _ = _forward(net, graph)
    _scale_region(net, dims, "w", j, 1)
    z1, s1 = _forward(net, graph)
    assert int((z1 != z0).sum()) > 0, f"layer {j}: z does not depend on the packed copy"
    want_z, want_s = _forward(_net(hp, W.doubled(p, 1, j), False), graph)
    _assert_same_bits(f"route, Wp_{j} doubled vs generic tile on 2 W_{j}", {"z": z1, "sums": s1}, {"z": want_z, "sums": want_s})


def test_route_seven_inputs_stay_on_the_generic_tile():
    """in = 7 is no whole float4: launch_linear_short refuses it (gnf_common.h: linear_short_fwd_layer) - doubling Wp_0
    changes nothing, while the middle layer of the same net still follows its packed copy."""
    hp, dims, p, graph = _route_setup(14, 1280, act="leaky_relu")
    assert W.short_deal(ROUTE_N, dims[0], dims[1], _cus()) is None
    net = _net(hp, p, True)
    z0, _ = _forward(net, graph)
    _scale_region(net, dims, "w", 0, 0)
    z1, _ = _forward(net, graph)
    assert torch.equal(z1, z0), "a 7-input first layer read its packed copy"
    _scale_region(net, dims, "w", 1, 0)
    z2, _ = _forward(net, graph)
    assert int((z2 != z0).sum()) > 0


@pytest.mark.parametrize("latent", [1280, 1040])
@pytest.mark.parametrize("stash", [True, False], ids=["stash", "recompute"])
def test_route_backward_dx_reads_the_transposed_copy(stash, latent):
    """Doubling WpT_1 of half-step 1's nets doubles dP_0 = (dP_1 W_1^T) * act'(h_1) exactly: dW_0 and db_0 of those two nets
    come out exactly 2 x, every gradient of their layers 1 and 2 keeps its bits; with fused = False nothing changes.
    At latent 1040 the forward pass is the LDS-resident kernel's and this walk is all the wide kernels see of the net."""
    hp, dims, p, graph = _route_setup(200, latent, lds_forward=latent == 1040)
    for fused in (True, False):
        tr, _ = _train(hp, p, graph, fused, stash)
        g0 = tr.grad.clone()
        tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        assert torch.equal(tr.grad, g0), "two calls differ: nothing can be proved by a change"
        _scale_region(tr.net, dims, "wt", 1, 1)
        tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        g1 = tr.grad.clone()
        if not fused:
            assert torch.equal(g1, g0), "fused = False read the packed buffer"
            continue
        for name, sl in _grad_tensors(tr, hp):
            if name[:4] not in ("s[1]", "t[1]"):
                continue
            if name.endswith("0"):
                assert float(g0[sl].abs().max()) > 0
                assert torch.equal(g1[sl], 2.0 * g0[sl]), f"{name} is not exactly twice what it was: dX of layer 1 did not read WpT_1"
            else:
                assert torch.equal(g1[sl], g0[sl]), f"{name} changed with WpT_1"
        other = torch.cat([g1[sl] != g0[sl] for name, sl in _grad_tensors(tr, hp) if name[:4] in ("s[0]", "t[0]")])
        print(f"[wide] route backward ({'stash' if stash else 'recompute'}): {int(other.sum())} gradient elements of the other half-step follow dX")


def test_route_backward_dx_without_a_mask_reads_the_transposed_copy():
    """D = 512, agg: in0 = 256, so dX of layer 0 is the transposed k_linear_big with aux == NULL and ONE column block.
    Doubling WpT_0 of every net changes gradients (the input gradient of a half-step feeds the walk's next half-step) and
    none of the doubled nets' own layer-0 gradients; fused = False: nothing."""
    n = NO_MASK_N[512]
    hp, dims, p, graph = _route_setup(512, 1280, n=n)
    assert W.big_bwd_layer(dims[0], dims[1]) and W.pad16(dims[0]) == 256 and W.big_deal(n, dims[0], _cus())
    for fused in (True, False):
        tr, _ = _train(hp, p, graph, fused, False)
        g0 = tr.grad.clone()
        for half in (0, 1):
            _scale_region(tr.net, dims, "wt", 0, half)
        tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        changed = int((tr.grad != g0).sum())
        print(f"[wide] route backward, no mask (fused = {fused}): {changed} gradient elements follow WpT_0")
        assert (changed > 0) == fused


# ---------------------------------------------------------------------------------------------------------------------------
# 2, 3, 4. Row deals and shapes: every direction of the wide route against the generic tile, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def _parity(label, hp, n, seed=62):
    graph = _graph(n, hp["D"])[0]
    p = W.make_params(hp, seed)
    wide = _everything(hp, p, graph, True)
    gen = _everything(hp, p, graph, False, z_for_inverse=wide["z"])
    _assert_same_bits(label, wide, gen)


BIG_DEALS = [   # row tiles, rows, (wg_base, wg_rem) on 256 CUs at 10 panels, workgroup sizes reached, rounds
    (103, 1640, (1, 51), {1, 2}, 1),
    (104, 1664, (2, 0), {2}, 1),
    (130, 2080, (2, 26), {2, 3}, 1),
    (156, 2496, (3, 0), {3}, 1),
    (204, 3257, (3, 48), {3, 4}, 1),
    (205, 3280, (1, 102), {1, 2}, 2),
]


@pytest.mark.parametrize("tiles,n,deal,sizes,rounds", BIG_DEALS, ids=[f"rt{c[0]}_n{c[1]}" for c in BIG_DEALS])
def test_k_linear_big_row_deals_give_the_generic_tiles_bits(tiles, n, deal, sizes, rounds):
    """D = 300 (H = 150: neither the short first layer nor the thin last one), latent 1280: the middle layer and its dX are
    k_linear_big's, everything else the generic tile's on both routes."""
    got = W.big_deal(n, 1280, _cus())
    assert got is not None and (got["n_rt"], got["wg_base"], got["wg_rem"], got["sizes"], got["rounds"]) == \
        (tiles, deal[0], deal[1], sizes, rounds), f"this chip deals {got}: the case would test something else"
    hp = W.make_hp(300, 1280)
    dims = W.net_dims(300, 1280, 3, "agg")
    assert not W.short_fwd_layer(dims[0], dims[1]) and not W.fused_last(dims, 2) and not W.fused_fwd_fits(dims)
    _parity(f"k_linear_big rt{tiles}", hp, n)


SHORT_DEALS = [   # rows, (wg_base, wg_rem), rounds of k_linear_short<11,2> (144 -> 1280: 20 panels) on 256 CUs
    (1640, (3, 25), 1),
    (6560, (7, 46), 2),
]


@pytest.mark.parametrize("n,deal,rounds", SHORT_DEALS, ids=[f"n{c[0]}" for c in SHORT_DEALS])
def test_k_linear_short_row_deals_give_the_generic_tiles_bits(n, deal, rounds):
    got = W.short_deal(n, 144, 1280, _cus())
    assert got is not None and (got["wg_base"], got["wg_rem"], got["rounds"]) == (deal[0], deal[1], rounds), \
        f"this chip deals {got}: the case would test something else"
    assert W.big_deal(n, 1280, _cus()) is not None
    _parity(f"k_linear_short n{n}", W.make_hp(288, 1280), n)


def _all_big(dims, n):
    """every layer of the net is k_linear_big's in both directions, on this chip and this batch"""
    cus = _cus()
    return all(W.big_fwd_layer(i, o) and W.big_bwd_layer(i, o) and W.big_deal(n, o, cus) and W.big_deal(n, i, cus)
               for i, o in zip(dims[:-1], dims[1:]))


@pytest.mark.parametrize("latent,act", [(512, "relu"), (528, "leaky_relu"), (1030, "relu"), (1040, "relu")],
                         ids=["L512", "L528", "L1030", "L1040"])
def test_k_linear_big_width_edges_give_the_generic_tiles_bits(latent, act):
    """Hidden widths below about 1130 fit the LDS-resident kernels unless another width of the net is larger; with D = 2400
    (H = 1200) the flow is layered and ALL THREE layers are k_linear_big's, forward (the last one without activation) and
    transposed (layer 0 without a mask, 75 k-groups: four chunks and an odd rest)."""
    n = 4090
    dims = W.net_dims(2400, latent, 3, "agg")
    assert not W.fused_fwd_fits(dims) and not W.fused_bwd_fits(dims) and _all_big(dims, n)
    _parity(f"k_linear_big L{latent}", W.make_hp(2400, latent, act=act), n, seed=63)


@pytest.mark.parametrize("d,latent,act,combine,n", [(300, 1280, "leaky_relu", "agg", 3257), (512, 1280, "relu", "agg", NO_MASK_N[512]),
                                                    (300, 1280, "relu", "concat", NO_MASK_N[300])],
                         ids=["L1280_leaky", "in256_no_mask", "in300_no_mask"])
def test_k_linear_big_activations_and_unmasked_dx_give_the_generic_tiles_bits(d, latent, act, combine, n):
    """leaky_relu through the forward epilogue and the act' mask; dX of a first layer with at least 256 inputs (the transposed
    product with aux == NULL: 256 inputs = one column block, 300 = two with a ragged second)."""
    dims = W.net_dims(d, latent, 3, combine)
    assert W.big_deal(n, latent, _cus()) and not W.fused_fwd_fits(dims) and not W.fused_bwd_fits(dims) and not W.fused_last(dims, 2)
    assert not W.big_bwd_layer(dims[0], dims[1]) or W.big_deal(n, dims[0], _cus())
    _parity(f"k_linear_big D{d} L{latent} {act} {combine}", W.make_hp(d, latent, act=act, combine=combine), n, seed=64)


SHORT_INPUTS = [   # in, instance, k-groups, hidden width
    (4, "7x4", 1, 1296), (100, "7x4", 7, 1296), (128, "8x4", 8, 1296), (144, "11x2", 9, 1296), (176, "11x2", 11, 1296),
    (164, "11x2", 11, 1296), (208, "13x2", 13, 1296), (100, "7x4", 7, 1280),
]


@pytest.mark.parametrize("inw,inst,kgs,latent", SHORT_INPUTS, ids=[f"in{c[0]}_L{c[3]}" for c in SHORT_INPUTS])
def test_k_linear_short_input_widths_give_the_generic_tiles_bits(inw, inst, kgs, latent):
    """K = 2 nets in -> latent -> in (agg): the first layer is k_linear_short's and nothing else differs between the routes
    (no middle layer for k_linear_big, a last layer the generic tile runs on both).  1296 = 81 column tiles: the last column
    block of either instance has one live tile."""
    n = 1664
    dims = W.net_dims(2 * inw, latent, 2, "agg")
    got = W.short_deal(n, inw, latent, _cus())
    assert got is not None and (got["instance"], got["ipg"]) == (inst, kgs) and not W.fused_fwd_fits(dims)
    _parity(f"k_linear_short in{inw} L{latent}", W.make_hp(2 * inw, latent, k=2), n, seed=65)


# ---------------------------------------------------------------------------------------------------------------------------
# The thin last layer out of the accumulators: not bitwise by design - both routes against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _flat(grads):
    for kind in ("s", "t"):
        for q, net in enumerate(grads[kind][0] + grads[kind][1]):
            for j, (w, b) in enumerate(net):
                yield f"{kind}[{q}].W{j}", w
                yield f"{kind}[{q}].b{j}", b


ORACLE_CASES = [   # D, latent, activation, what keeps the case from being bitwise
    (130, 1280, "leaky_relu", "thin_last"),     # H = 65: five thin column tiles, the second pass has one live tile and cw = 1
    (200, 1280, "relu", "thin_last"),           # H = 100
    (200, 1296, "relu", "thin_last"),           # 81 column tiles: the last column block feeds ONE k-group into the thin layer
    (300, 1040, "relu", "lds_forward"),         # forward and inverse in k_half_fused, the backward walk in k_linear_big
]


@pytest.mark.parametrize("d,latent,act,why", ORACLE_CASES, ids=[f"D{c[0]}_L{c[1]}_{c[3]}" for c in ORACLE_CASES])
def test_routes_that_are_not_bitwise_vs_fp64_oracle(d, latent, act, why):
    """Both routes against the float64 oracle: z and the round trip within SLACK x the float32 restatement's own error +
    FLOOR (tests/test_fullsize_gpu.py); every gradient tensor of the thin_last cases, in both stash modes, under the two-norm
    rule of test_wide_layer_takes_the_thin_last_layer_along (2e-3 of the tensor's norm).  The lds_forward case is this
    module's own and compares z, the round trip and the loss only: on its inputs one hidden unit lies within rounding of its
    relu's kink, the float32 autograd of the oracle itself is 2.3e-3 off in ds[0].W0 with one BLAS blocking and 7e-4 with
    another, and every device route, the generic one included, reads 2.3e-3 - no bound derived from a CPU run holds on
    every host.  What the wide kernels do in that net's backward walk is pinned exactly: the 2 x proof above, and the same
    width bit for bit in test_k_linear_big_width_edges_give_the_generic_tiles_bits."""
    n = 1664
    hp = W.make_hp(d, latent, act=act)
    dims = W.net_dims(d, latent, 3, "agg")
    assert W.big_deal(n, latent, _cus()) and not W.fused_bwd_fits(dims)
    if why == "thin_last":
        assert W.fused_last(dims, 2) and not W.fused_fwd_fits(dims)
    else:
        assert W.fused_fwd_fits(dims) and not W.fused_last(dims, 2)
    graph, (nn, ne, s, r), x = _graph(n, d)
    p = W.make_params(hp, 66)
    c = _conditioning(hp, s, r, n, x, p)
    ref = O.loss_and_grads(s, r, n, x, p, 1, activation=act, combine="agg", epsilon=1.0)
    gmax = max(float(np.abs(b).max()) for _, b in _flat(ref["grads"]))

    def rel_bound(g):   # a tensor's two-norm, a gradient that is zero by cancellation judged against the flow's scale
        return max(float(np.linalg.norm(g)), 1e-3 * gmax * np.sqrt(g.size))
    worst = []
    zs = {}
    for fused in (True, False):
        tag = f"D{d} L{latent} {'wide' if fused else 'generic'}"
        net = _net(hp, p, fused)
        z, _ = _forward(net, graph)
        zs[fused] = z
        z_err = float((z.cpu().double() - c["ref"]["z"]).abs().max())
        back = net(graph.replace(nodes=z), inverse=False).nodes
        rt = float((back - graph.nodes).abs().max())
        ratios = [("z", z_err / (SLACK * c["z_err32"] + FLOOR)), ("round trip", rt / (SLACK * c["rt_err32"] + FLOOR))]
        for stash in (True, False):
            tr, out = _train(hp, p, graph, fused, stash)
            assert abs(float(out["total_loss"]) - ref["total_loss"]) <= 1e-4 * n
            if why != "thin_last":
                continue
            per = []
            for (name, a), (_, g) in zip(_flat(tr.named_gradients()), _flat(ref["grads"])):
                per.append((f"d{name}", float(np.linalg.norm(a - g)) / (2e-3 * rel_bound(g))))
            name, ratio = max(per, key=lambda v: v[1])
            ratios.append((f"worst gradient, {'stash' if stash else 'recompute'} ({name})", ratio))
        for name, ratio in ratios:
            print(f"[wide] oracle {tag}: {name}: {ratio:.3f} of its bound")
        worst += [(tag, name, ratio) for name, ratio in ratios]
    assert not torch.equal(zs[True], zs[False]), "the two routes give the same bits: this case belongs to the bitwise tests"
    for tag, name, ratio in worst:
        assert ratio <= 1.0, (tag, name, ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. The re-pack after an optimiser step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,latent", [(200, 1040), (24, 1280), (14, 1030)], ids=["D200_L1040", "D24_L1280", "D14_L1030"])
def test_repack_after_optimiser_steps_equals_a_fresh_pack(d, latent):
    """k_pack_multi (gnf_optim.hip) after two steps against gnf_pack_mlp of a fresh net with the same weights: Wp_j where a
    kernel reads it, WpT_j likewise, every padded bias row - bit for bit."""
    from gnf_amd.train import GRevNetTrainer
    n = 1664
    hp = W.make_hp(d, latent)
    dims = W.net_dims(d, latent, 3, "agg")
    graph = _graph(n, d)[0]
    net = _net(hp, W.make_params(hp, 67), True)
    tr = GRevNetTrainer(net, lr=2e-3, use_lr_decay=False)
    first = None
    for _ in range(2):
        tr.step(graph)
        torch.cuda.synchronize()
        first = _packed(net).clone() if first is None else first
    stepped = _packed(net).clone()
    assert not torch.equal(stepped, first), "the second step did not move the packed copy: the test would prove nothing"
    fresh_net = _net(hp, net.get_params(), True)
    _forward(fresh_net, graph)
    fresh = _packed(fresh_net)
    per_net = W.packed_floats(dims)
    assert stepped.numel() == fresh.numel() == 4 * per_net
    compared, stale = 0, []
    for q in range(4):
        for j in range(3):
            kinds = ["b"] + (["w"] if W.need_w(dims, j) else []) + (["wt"] if W.need_wt(dims, j) else [])
            for kind in kinds:
                off, ln = W.packed_region(dims, kind, j)
                a, b = stepped[q * per_net + off:q * per_net + off + ln], fresh[q * per_net + off:q * per_net + off + ln]
                compared += 1
                if not torch.equal(a, b):
                    stale.append((q, kind, j, int((a != b).sum())))
    print(f"[wide] re-pack D{d} L{latent}: wide_only = {W.wide_only(dims)}, {compared} regions compared, stale: {stale}")
    assert not stale, stale
