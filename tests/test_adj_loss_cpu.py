"""gnf_amd.adj_loss.binary_loss / gnf_adj_loss_f32: everything that needs no GPU - the float64 restatement the GPU tests compare
against (its literal loss.py form against its logit-space form, its gradient against central differences, the clip's zero
gradient), the margin condition on every batch the GPU tests use, the symbols, the host-side workspace size, the argument
validation before any launch and the Python layer's argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gnf_amd import _abi

import adj_loss_ref as R

NEW_SYMBOLS = ("gnf_adj_loss_workspace_bytes", "gnf_adj_loss_f32")
P = 0x1000   # a non-null pointer that validation never dereferences
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
GPU_DIMS = (1, 2, 7, 64, 200, 400, 1030)   # tests/test_adj_loss_gpu.py: 400 is the width that keeps only the row tile in LDS


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dist,soft", [(7, R.SCALED_HACKY, False), (7, R.SCALED_HACKY, True), (2, R.HACKY, False),
                                         (64, R.sigmoid_l2(3.0, 2.0), True), (7, R.sigmoid_l2(20.0, 1.0), False)])
def test_literal_form_equals_logit_form(d, dist, soft):
    z = R.embeddings(R.SIZES, d, 0, duplicate_rows=True)
    _, s, r = R.true_graph(R.SIZES, 0)
    ref = R.binary_loss(z, R.SIZES, s, r, dist, soft)
    total, mean, masked = R.binary_loss_literal(z, R.SIZES, s, r, dist, soft)
    n = sum(R.SIZES)
    assert ref["sum_loss"] > 100.0
    assert abs(total - ref["sum_loss"]) <= 1e-9 * ref["sum_loss"] and abs(mean - ref["mean_loss"]) <= 1e-9 * ref["mean_loss"]
    assert ref["mean_loss"] == ref["sum_loss"] / (n * n - n)
    for b, want in zip(ref["blocks"], ref["loss_per_graph"]):
        o, ng = b["n0"], b["ng"]
        assert abs(masked[o:o + ng, o:o + ng].sum() - want) <= 1e-9 * want
        masked[o:o + ng, o:o + ng] = 0.0
    assert not masked.any()                                          # nothing outside the graphs' blocks
    assert ref["loss_per_graph"][0] == 0.0 == ref["loss_per_graph"][1]   # the 1-node and the empty graph
    clipped = sum(int(b["clipped"].sum()) for b in ref["blocks"])
    assert clipped > 0                                               # the clip is exercised (lower, and upper at temp = 20)
    if dist[0] == 20.0:
        assert any((b["clipped"] & (b["u"] > R.U)).any() for b in ref["blocks"])


def test_labels_self_loops_duplicates_and_foreign_edges():
    sizes = [3, 2]
    # 0 -> 1 twice, a self loop, an edge into the other graph, 3 -> 4
    s, r = np.array([0, 0, 2, 1, 3]), np.array([1, 1, 2, 3, 4])
    z = R.embeddings(sizes, 2, 0)
    blocks = R.graph_blocks(z, sizes, s, r)
    assert blocks[0]["a"].astype(int).tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]]
    assert blocks[1]["a"].astype(int).tolist() == [[0, 1], [0, 0]]
    ref = R.binary_loss(z, sizes, s, r)
    only = R.binary_loss(z, sizes, np.array([0, 3]), np.array([1, 4]))
    assert ref["sum_loss"] == only["sum_loss"] and np.array_equal(ref["grad"], only["grad"])
    # the counts are ordered pairs with |p - a| > abs_tol, by sign
    p, a = blocks[0]["u"] > 0, blocks[0]["a"]
    assert ref["fp"][0] == (p & ~a & blocks[0]["off"]).sum() and ref["fn"][0] == (~p & a).sum()


def _small_batch():
    """sizes [5, 1, 9] at D = 3 with every |u| at least 1e-3 from +-U, so a step of 1e-6 crosses no kink"""
    sizes = [5, 1, 9]
    _, s, r = R.true_graph(sizes, 3, duplicates=1)
    for seed in range(16):
        z = R.embeddings(sizes, 3, seed).astype(np.float64)
        z[5 + 1 + 2] *= 3.0   # (a far node: clipped pairs)
        blocks = R.graph_blocks(z, sizes, s, r)
        if all((np.abs(np.abs(b["u"]) - R.U) > 1e-3)[b["off"]].all() for b in blocks):
            return sizes, z, s, r
    raise AssertionError("no seed in range(16) keeps the small batch off the clip's kinks")


@pytest.mark.parametrize("dist,soft", [(R.SCALED_HACKY, False), (R.SCALED_HACKY, True), (R.HACKY, False),
                                       (R.sigmoid_l2(3.0, 2.0), False)])
def test_gradient_equals_central_differences(dist, soft):
    sizes, z, s, r = _small_batch()
    ref = R.binary_loss(z, sizes, s, r, dist, soft)
    assert any(b["clipped"].any() for b in ref["blocks"]) and np.abs(ref["grad"]).max() > 0.1
    h, fd = 1e-6, np.zeros_like(z)
    for i in range(z.shape[0]):
        for f in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[i, f] += h
            zm[i, f] -= h
            fd[i, f] = (R.binary_loss(zp, sizes, s, r, dist, soft)["sum_loss"] -
                        R.binary_loss(zm, sizes, s, r, dist, soft)["sum_loss"]) / (2.0 * h)
    # roundoff of a loss of a few hundred over 2e-6, truncation h^2 f''': both far below 1e-6 of the gradient's scale
    assert np.abs(fd - ref["grad"]).max() <= 1e-6 * np.abs(ref["grad"]).max()
    assert not ref["grad"][5].any()                                  # the 1-node graph


def test_clipped_pairs_contribute_exactly_zero_gradient():
    # a true edge whose endpoints lie far apart, both directions: u < -U, the loss is the constant U, the gradient exactly 0
    z = np.array([[0.0, 0.0], [3.0, 1.0]])
    s, r = np.array([0, 1]), np.array([1, 0])
    ref = R.binary_loss(z, [2], s, r)
    assert ref["blocks"][0]["clipped"].sum() == 2 and ref["sum_loss"] == pytest.approx(2.0 * R.softplus(R.U), rel=1e-15)
    assert not ref["grad"].any() and ref["fn"][0] == 2
    moved = R.binary_loss(z + np.array([[1e-3, 0.0], [0.0, -1e-3]]), [2], s, r)
    assert moved["sum_loss"] == ref["sum_loss"]                      # and finite differences see exactly 0 as well
    # in a mixed batch the gradient is the sum over the pairs the clip leaves alone
    sizes, zz, s, r = _small_batch()
    ref = R.binary_loss(zz, sizes, s, r)
    for b in ref["blocks"]:
        assert not b["c"][b["clipped"]].any()
        if b["ng"] == 9:
            assert b["clipped"].any() and (b["a"] & b["clipped"]).any()   # true edges among them
            zg = zz[b["n0"]:b["n0"] + 9]
            manual = np.zeros_like(zg)
            for i in range(9):
                for j in range(9):
                    if i != j and not b["clipped"][i, j]:
                        t_ij, t_ji = float(b["a"][i, j]), float(b["a"][j, i])
                        manual[i] += -2.0 * 10.0 / np.sqrt(3.0) * ((b["p"][i, j] - t_ij) + (b["p"][i, j] - t_ji)) * (zg[i] - zg[j])
            np.testing.assert_allclose(ref["grad"][b["n0"]:b["n0"] + 9], manual, rtol=1e-12, atol=1e-12)


# ---- the margin condition on the GPU tests' inputs -------------------------------------------------------------------------
@pytest.mark.parametrize("d", GPU_DIMS)
def test_a_seed_with_margin_exists_for_every_width(d):
    seed, z, (n_edge, s, r) = R.pick_seed(R.SIZES, d)
    assert seed is not None, f"D={d}: no seed in range(16) keeps every pair 2 delta from the kinks"
    assert z.dtype == np.float32 and z.shape == (198, d) and int(n_edge.sum()) == len(s) == len(r)
    ref = R.binary_loss(z, R.SIZES, s, r)
    pairs = sum(ng * ng - ng for ng in R.SIZES)
    clipped = sum(int(b["clipped"].sum()) for b in ref["blocks"]) / pairs
    positive = sum(int(((b["u"] > 0) & b["off"]).sum()) for b in ref["blocks"]) / pairs
    print(f"D={d}: seed {seed}, {100 * clipped:.1f} % of the pairs clipped, {100 * positive:.1f} % with p > 0.5")
    assert 0.02 < clipped < 0.6 and 0.3 < positive < 0.95             # every branch sees many pairs
    assert ref["fp"].sum() > 100 and ref["fn"].sum() > 100


def test_a_seed_with_margin_exists_for_the_other_batches():
    for dist, dup in ((R.HACKY, False), (R.sigmoid_l2(3.0, 2.0), False), (R.sigmoid_l2(20.0, 1.0), True)):
        seed, z, (_, s, r) = R.pick_seed(R.SIZES, 7, dist, duplicate_rows=dup)
        assert seed is not None, dist
        if dup:   # two identical rows: u = temp * shift = 20 > U
            ref = R.binary_loss(z, R.SIZES, s, r, dist)
            b = ref["blocks"][2]
            assert b["u"][0, 1] == 20.0 > R.U and b["clipped"][0, 1] and b["c"][0, 1] == 0.0
    assert R.pick_seed(R.SIZES, 7, symmetric=True)[0] is not None
    assert R.pick_seed([300, 3], 16)[0] is not None


# ---- ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    """include/gnf_adj_loss.h (included by gnf.h), the library's exports and _abi.ADJ_LOSS_SYMBOLS are in step"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_adj_loss.h"$', main, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_adj_loss.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.ADJ_LOSS_SYMBOLS)
    assert not set(_abi.ADJ_LOSS_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS)
    assert not set(_abi.ADJ_LOSS_SYMBOLS) & set(_abi.ORBIT_SYMBOLS)
    assert len(_abi.EXPORTED_SYMBOLS) == 41
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    assert C.sizeof(_abi.GnfAdjLossSpec) == 24


def test_workspace_size_is_a_host_computation_and_monotone():
    ws = _abi.lib().gnf_adj_loss_workspace_bytes
    # two bitmaps [N][ceil(max / 64)] uint64 | row loss fp64 [N] | row fp, fn counts int32 [N] each
    assert ws(4, 100, 64) == 2 * 100 * 1 * 8 + 100 * 8 + 2 * 100 * 4
    assert ws(4, 100, 65) == 2 * 100 * 2 * 8 + 100 * 8 + 2 * 100 * 4
    assert ws(4, 101, 64) > ws(4, 100, 64) and ws(4, 100, 63) <= ws(4, 100, 64) and ws(4, 101, 64) % 8 == 0
    for a, b in ((1, 2), (7, 300), (300, 301), (0, 65536)):
        assert ws(a, 50, 40) <= ws(b, 50, 40) and ws(3, a, 40) <= ws(3, b, 40) and ws(3, 50, a) <= ws(3, 50, b)
    assert ws(-1, 10, 10) == 0 and ws(3, -1, 10) == 0 and ws(3, 10, -1) == 0 and ws(0, 0, 0) == 0


def _csr(n=40, e=100, b=3, off=P, rowptr=P, col=P):
    return _abi.GnfCsr(rowptr, col, n, e, off, b)


def _spec(temp=10.0, shift=1.0, by_sqrt=1, soft=0, eps=0.1, tol=0.5):
    return _abi.GnfAdjLossSpec(temp, shift, by_sqrt, soft, eps, tol)


def _call(csr=None, z=P, ld=8, d=8, cap=20, spec=None, loss=P, sums=P, fp=P, fn=P, grad=P, ldg=8, scale=1.0, ws=P,
          ws_bytes=1 << 20):
    csr = _csr() if csr is None else csr
    spec = _spec() if spec is None else spec
    return _abi.lib().gnf_adj_loss_f32(C.byref(csr), z, ld, d, cap, C.byref(spec), loss, sums, fp, fn, grad, ldg, scale, ws,
                                       ws_bytes, None)


def test_validation_without_a_gpu():
    lib = _abi.lib()
    err = lambda: lib.gnf_last_error().decode()
    # GNF_EINVAL: null pointers, missing node_offsets
    assert _call(csr=_csr(off=None)) == EINVAL and "node_offsets" in err()
    assert _call(csr=_csr(b=0)) == EINVAL
    assert lib.gnf_adj_loss_f32(None, P, 8, 8, 20, C.byref(_spec()), P, P, P, P, P, 8, 1.0, P, 1 << 20, None) == EINVAL
    assert lib.gnf_adj_loss_f32(C.byref(_csr()), P, 8, 8, 20, None, P, P, P, P, P, 8, 1.0, P, 1 << 20, None) == EINVAL
    for name in ("z", "loss", "sums", "fp", "fn", "ws"):
        assert _call(**{name: None}) == EINVAL, name
    assert _call(csr=_csr(rowptr=None)) == EINVAL and _call(csr=_csr(col=None)) == EINVAL
    # GNF_ESHAPE: D < 1, ld < D, ld_grad < D, negative sizes, a cap out of range, label_epsilon outside [0, 0.5], abs_tol < 0
    assert _call(d=0) == ESHAPE and _call(d=-3) == ESHAPE and _call(ld=7) == ESHAPE and "ld" in err()
    assert _call(ldg=7) == ESHAPE
    assert _call(csr=_csr(n=-1)) == ESHAPE and _call(csr=_csr(e=-1)) == ESHAPE and _call(csr=_csr(b=-1)) == ESHAPE
    assert _call(cap=-1) == ESHAPE and _call(cap=65537) == ESHAPE and _call(cap=0) == ESHAPE
    for eps in (-0.01, 0.51, float("nan")):
        assert _call(spec=_spec(eps=eps)) == ESHAPE and "label_epsilon" in err()
    assert _call(spec=_spec(tol=-0.1)) == ESHAPE and _call(spec=_spec(tol=float("nan"))) == ESHAPE
    # GNF_EWORKSPACE - the last check, so it also shows which values pass the ones before it (a call that passed them all
    # would launch on these fake pointers: every call here fails one)
    need = lib.gnf_adj_loss_workspace_bytes(3, 40, 20)
    assert _call(ws_bytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert _call(ldg=7, grad=None, ws_bytes=need - 1) == EWORKSPACE   # no gradient: ld_grad is not read
    for eps, tol in ((0.0, 0.0), (0.5, 0.5), (0.1, 3.0)):
        assert _call(spec=_spec(eps=eps, tol=tol), ws_bytes=need - 1) == EWORKSPACE
    assert _call(cap=65536, ws_bytes=need) == EWORKSPACE             # the bound itself is accepted, its bitmaps are larger


def test_python_layer_argument_errors():
    import gnf_amd
    from helpers import graph_from_arrays
    from gnf_amd import adj_loss
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    assert gnf_amd.binary_loss is adj_loss.binary_loss and gnf_amd.sigmoid_l2 is adj_loss.sigmoid_l2
    assert gnf_amd.hacky_sigmoid_l2 is adj_loss.hacky_sigmoid_l2
    g = graph_from_arrays([3], [2], [0, 1], [1, 2], np.zeros((3, 4), np.float32))
    for kw in ({}, {"max_nodes_per_graph": 3}, {"grad": "sum"}, {"distance_fn": adj_loss.sigmoid_l2(3.0, 2.0)},
               {"distance_fn": adj_loss.hacky_sigmoid_l2}, {"distance_fn": scaled_hacky_sigmoid_l2}):
        with pytest.raises(_abi.GnfError):                           # CPU tensors: no fallback
            adj_loss.binary_loss(g, g, **kw)
    with pytest.raises(NotImplementedError):
        adj_loss.binary_loss(g, g, distance_fn=lambda nodes: nodes)
    with pytest.raises(NotImplementedError):
        adj_loss.binary_loss(g, g, distance_fn=adj_loss.sigmoid_l2)      # the class, not a token made from it
    with pytest.raises(NotImplementedError):
        adj_loss.hacky_sigmoid_l2(g.nodes)
    other = graph_from_arrays([4], [0], [], [], np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        adj_loss.binary_loss(other, g)                               # node totals differ
    for kw in ({"grad": "both"}, {"epsilon": 0.6}, {"epsilon": -0.1}, {"abs_tol": -1.0}):
        with pytest.raises(ValueError):
            adj_loss.binary_loss(g, g, **kw)
    tok = adj_loss.sigmoid_l2(3, 2)
    assert (tok.temp, tok.shift) == (3.0, 2.0) and adj_loss._distance_params(tok) == (3.0, 2.0, 1)
    assert adj_loss._distance_params(adj_loss.hacky_sigmoid_l2) == (10.0, 1.0, 0)
    assert adj_loss._distance_params(scaled_hacky_sigmoid_l2) == (10.0, 1.0, 1)
    # the host helpers of loss.py:88-116 over a result dict: the ordered-pair counts halved
    res = {"false_positive_pairs": torch.tensor([4, 0, 6]), "false_negative_pairs": torch.tensor([2, 0, 1])}
    per_graph = adj_loss.incorrect_edges_per_graph(res)
    assert per_graph.dtype == torch.int32 and per_graph.tolist() == [3, 0, 3]
    for fn, want in ((adj_loss.false_positive_edges, 5.0), (adj_loss.false_negative_edges, 1.5),
                     (adj_loss.total_incorrect_edges, 6.5)):
        got = fn(res)
        assert got.dtype == torch.float64 and got.dim() == 0 and float(got) == want
