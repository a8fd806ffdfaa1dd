"""gnf_amd.triplet_loss.triplet_loss (gnf_triplet_loss_f32) on the MI355X against the restatement of tests/triplet_loss_ref.py.

Batch: graphs of [1, 0, 17, 16, 33, 65, 2, 64, 130] nodes from adj_loss_ref.true_graph (directed, duplicated edges, rows of up to
3 bitmap words), self loops on every other node, then a complete graph of 9 nodes (no negatives) and an edgeless one of 5 (no
positives).  The embeddings and the hash share the first seed in range(16) whose terms keep their gap from every kink
(triplet_loss_ref.pick_seed; tests/test_triplet_loss_cpu.py asserts that such a seed exists).

Integers are EQUAL: pos_index, neg_index and skipped_terms are those of the restatement's Python-integer hash and candidate rule.
Floats are held against float64 under triplet_loss_ref.bounds: 4 x the float32 restatement's own distance from float64 plus
16 fp32 ulp of the output's largest entry, per output.  Every ratio is printed before it is asserted (pytest -s).

The implementation has one route.  Sizes at which a loop takes another turn: a row of more than 64 edges (the 130-node graph),
more than 64 bitmap words (the rings of 4096 and 4161 nodes: the prefix scan's second chunk), a graph whose 2 L n records fill
more than one chunk of the counting sort (all but the smallest), D above 64 (the gradient's second feature chunk)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import triplet_loss_ref as R
from helpers import GuardBanded, graph_from_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("sum_loss", "mean_loss", "loss_per_node", "loss_per_graph", "skipped_terms")
WIDTHS = (1, 3, 64, 100, 257)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _tokens(name, loss):
    from gnf_amd import adj_loss
    from gnf_amd.triplet_loss import dot, exp_l2, hacky_cauchy_l2, l2, margin_loss, relative_loss, sigmoid_dot
    fn = {"l2": l2, "dot": dot, "exp_l2": exp_l2, "hacky_sigmoid_l2": adj_loss.hacky_sigmoid_l2, "hacky_cauchy_l2": hacky_cauchy_l2,
          "sigmoid_dot": sigmoid_dot}[name]
    return fn, (margin_loss(loss[1]) if loss[0] == "margin" else relative_loss)


@functools.lru_cache(maxsize=None)
def _true_graph():
    sizes, n_edge, s, r = R.batch()
    return graph_from_arrays(sizes, n_edge, s, r, np.zeros((int(np.sum(sizes)), 1), np.float32), DEV)


def _emb(z, sizes=None):
    sizes = R.batch()[0] if sizes is None else sizes
    none = np.zeros(0, np.int32)
    return graph_from_arrays(sizes, np.zeros(len(sizes), np.int32), none, none, z, DEV)


def _hold(title, out, r64, r32, loops):
    """integers equal, floats under R.bounds; returns the largest error / bound"""
    n = len(r64["loss_per_node"])
    np.testing.assert_array_equal(out["pos_index"].cpu().numpy(), r64["pos"])
    np.testing.assert_array_equal(out["neg_index"].cpu().numpy(), r64["neg"])
    np.testing.assert_array_equal(out["skipped_terms"].cpu().numpy(), r64["skipped"])
    bd = R.bounds(r64, r32)
    got = {"loss_per_node": out["loss_per_node"], "loss_per_graph": out["loss_per_graph"], "sum_loss": out["sum_loss"],
           "grad": out["grad_nodes"]}
    worst, bad = 0.0, []
    for k in R.KEYS:
        err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - r64[k]).max(initial=0.0))
        ratio = err / bd[k] if bd[k] > 0 else (0.0 if err == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"[triplet] {title} {k}: err {err:.3e} bound {bd[k]:.3e} ratio {ratio:.3f}")
        if not err <= bd[k]:
            bad.append(f"{k}: err {err:.3e} > {bd[k]:.3e}")
    kept = n * loops - int(r64["skipped"].sum())
    assert kept > 0 and abs(float(out["mean_loss"]) - r64["mean_loss"]) <= bd["sum_loss"] / kept
    print(f"[triplet] {title}: worst ratio {worst:.3f}")
    assert not bad, title + "\n" + "\n".join(bad)
    return worst


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", ["keep", "skip"])
@pytest.mark.parametrize("loops", [1, 8])
@pytest.mark.parametrize("loss", [R.MARGIN, R.RELATIVE], ids=["margin", "relative"])
@pytest.mark.parametrize("name", list(R.SCORES))
@pytest.mark.parametrize("d", WIDTHS)
def test_parity_with_the_restatement(d, name, loss, loops, self_loops):
    from gnf_amd.triplet_loss import triplet_loss
    seed, z, r64, r32 = R.pick_seed(d, R.SCORES[name], loss, loops, self_loops)
    assert seed is not None, "no seed in range(16) satisfies the margin condition"
    fn, lf = _tokens(name, loss)
    emb, true = _emb(z), _true_graph()
    sizes = R.batch()[0]
    n, b = len(z), len(sizes)
    kw = dict(distance_fn=fn, triplet_loss_fn=lf, num_sampling_loops=loops, seed=seed, self_loops=self_loops)
    out = triplet_loss(emb, true, grad="sum", return_indices=True, **kw)
    plain = triplet_loss(emb, true, **kw)
    mean = triplet_loss(emb, true, grad="mean", n_node_host=sizes, **kw)
    assert set(plain) == set(KEYS) and set(out) == set(KEYS) | {"grad_nodes", "pos_index", "neg_index"}
    for k in KEYS:   # the gradient and the indices change no other output, nor do the sizes given on the host
        assert torch.equal(plain[k], out[k]) and torch.equal(mean[k], out[k]), k
    assert out["sum_loss"].dtype == torch.float64 and out["sum_loss"].dim() == 0 and out["mean_loss"].dim() == 0
    assert out["loss_per_node"].dtype == torch.float32 and out["loss_per_node"].shape == (n,)
    assert out["loss_per_graph"].dtype == torch.float64 and out["loss_per_graph"].shape == (b,)
    assert out["skipped_terms"].dtype == torch.int64 and out["skipped_terms"].shape == (b,)
    assert out["pos_index"].dtype == torch.int32 and out["pos_index"].shape == (loops, n) == out["neg_index"].shape
    assert out["grad_nodes"].dtype == torch.float32 and out["grad_nodes"].shape == (n, d)
    assert all(v.device.type == "cuda" for v in out.values())
    _hold(f"D={d} {name} {loss[0]} L={loops} {self_loops}", out, r64, r32, loops)
    g_sum, g_mean = out["grad_nodes"].cpu().numpy().astype(np.float64), mean["grad_nodes"].cpu().numpy().astype(np.float64)
    scale = float(np.abs(g_sum).max())
    assert scale > 0 and np.abs(g_mean * (n * loops) - g_sum).max() <= 2.0 ** -21 * scale    # one more fp32 product
    # the complete, the edgeless, the empty and the 1-node graph: every term skipped, zeros, no gradient
    for g in (0, 1, b - 2, b - 1):
        assert int(out["skipped_terms"][g]) == loops * sizes[g] and float(out["loss_per_graph"][g]) == 0.0
    assert not g_sum[0].any() and not g_sum[n - R.COMPLETE - R.EDGELESS:].any()
    assert not out["loss_per_node"][n - R.COMPLETE - R.EDGELESS:].any()


# ---- 2. the other sigmoid tokens, another margin ---------------------------------------------------------------------------
@pytest.mark.parametrize("score,token", [(R.SCALED_HACKY, "scaled"), (R.sigmoid_l2(3.0, 2.0), "sigmoid_l2")])
def test_the_scaled_sigmoid_tokens(score, token):
    from gnf_amd import adj_loss
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    from gnf_amd.triplet_loss import margin_loss, triplet_loss
    seed, z, r64, r32 = R.pick_seed(7, score, ("margin", 0.25), 4, "keep")
    assert seed is not None
    fn = scaled_hacky_sigmoid_l2 if token == "scaled" else adj_loss.sigmoid_l2(3.0, 2.0)
    out = triplet_loss(_emb(z), _true_graph(), fn, margin_loss(0.25), 4, seed=seed, grad="sum", return_indices=True)
    _hold(f"D=7 {token} margin 0.25", out, r64, r32, 4)


# ---- 3. draws ----------------------------------------------------------------------------------------------------------------
def test_given_draws_are_followed_and_the_hash_values_give_the_hash_bits():
    from gnf_amd.triplet_loss import exp_l2, relative_loss, triplet_loss
    sizes, _, s, r = R.batch()
    z = R.embeddings(sizes, 6, 1)
    n = len(z)
    emb, true = _emb(z), _true_graph()
    draws = np.random.default_rng(7).integers(0, 2 ** 32, size=(5, 2, n), dtype=np.uint64).astype(np.uint32)
    draws[0], draws[1] = 0, 2 ** 32 - 1                     # the first and the last candidate of every node
    for mode in ("keep", "skip"):
        pos, neg = R.sample(sizes, s, r, draws, mode)
        for t in (torch.as_tensor(draws.view(np.int32)).view(torch.uint32).to(DEV), torch.as_tensor(draws.astype(np.int64)).to(DEV)):
            out = triplet_loss(emb, true, num_sampling_loops=5, draws=t, self_loops=mode, return_indices=True)
            np.testing.assert_array_equal(out["pos_index"].cpu().numpy(), pos)
            np.testing.assert_array_equal(out["neg_index"].cpu().numpy(), neg)
    hashed = torch.as_tensor(R.hash_draws(123, 5, n).astype(np.int64)).to(DEV)
    kw = dict(distance_fn=exp_l2, triplet_loss_fn=relative_loss, num_sampling_loops=5, grad="sum", return_indices=True)
    a, b = triplet_loss(emb, true, seed=123, **kw), triplet_loss(emb, true, seed=99, draws=hashed, **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    other = triplet_loss(emb, true, seed=124, **kw)
    assert not torch.equal(a["pos_index"], other["pos_index"]) and not torch.equal(a["neg_index"], other["neg_index"])
    with pytest.raises(ValueError):
        triplet_loss(emb, true, num_sampling_loops=4, draws=hashed)
    with pytest.raises(ValueError):
        triplet_loss(emb, true, num_sampling_loops=5, draws=hashed.to(torch.float32))


# ---- 4. bit-reproducible; inputs are never written --------------------------------------------------------------------------
@pytest.mark.parametrize("d,name", [(64, "l2"), (257, "sigmoid_dot"), (3, "hacky_cauchy_l2")])
def test_two_calls_give_the_same_bits_and_inputs_are_not_written(d, name):
    from gnf_amd.graphs import csr_of
    from gnf_amd.triplet_loss import triplet_loss
    sizes = R.batch()[0]
    z = R.embeddings(sizes, d, 2)
    emb, true = _emb(z), _true_graph()
    fn, lf = _tokens(name, R.MARGIN)
    draws = torch.as_tensor(R.hash_draws(5, 8, len(z)).view(np.int32)).view(torch.uint32).to(DEV)
    csr = csr_of(true, by_sender=True)
    held = [emb.nodes, true.senders, true.receivers, true.n_node, true.n_edge, csr.rowptr, csr.col, draws.view(torch.int32)]
    before = [t.clone() for t in held]
    for kw in (dict(seed=5), dict(draws=draws)):
        first = triplet_loss(emb, true, fn, lf, grad="sum", return_indices=True, **kw)
        again = triplet_loss(emb, true, fn, lf, grad="sum", return_indices=True, **kw)
        for k in first:
            assert torch.equal(first[k], again[k]), k
        assert float(first["grad_nodes"].abs().max()) > 0 and bool(torch.isfinite(first["grad_nodes"]).all())
    for t, want in zip(held, before):
        assert torch.equal(t, want)


# ---- 5. strided embeddings, strided gradient: guard bands -------------------------------------------------------------------
def _raw(z_ptr, ld, d, true, spec, loops, grad_ptr=None, ldg=0, cap=130, draws=None):
    """gnf_triplet_loss_f32 itself: (loss_per_node, loss_per_graph, sums2, skipped, pos, neg)"""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lib = _abi.lib()
    n, b = int(true.nodes.shape[0]), int(true.n_node.shape[0])
    desc = csr_desc(true, csr_of(true, by_sender=True), node_offsets=True)
    outs = (torch.empty(n, dtype=torch.float32, device=DEV), torch.empty(b, dtype=torch.float64, device=DEV),
            torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(b, dtype=torch.int64, device=DEV),
            torch.empty((loops, n), dtype=torch.int32, device=DEV), torch.empty((loops, n), dtype=torch.int32, device=DEV))
    ws_bytes = lib.gnf_triplet_loss_workspace_bytes(b, n, loops)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.gnf_triplet_loss_f32(C.byref(desc), z_ptr, ld, d, cap, C.byref(spec), _abi.ptr(draws), *[_abi.ptr(t) for t in outs],
                                      grad_ptr, ldg, 1.0, _abi.ptr(ws), ws_bytes, _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("d,ld,c0,ldg,g0", [(3, 7, 1, 5, 2), (64, 72, 4, 64, 0), (100, 103, 3, 131, 31)])
def test_strided_buffers_are_bit_equal_and_guard_bands_stay(d, ld, c0, ldg, g0):
    from gnf_amd import _abi
    from gnf_amd.triplet_loss import hacky_cauchy_l2, relative_loss, triplet_loss
    sizes = R.batch()[0]
    z = R.embeddings(sizes, d, 3)
    n = len(z)
    emb, true = _emb(z), _true_graph()
    want = triplet_loss(emb, true, hacky_cauchy_l2, relative_loss, 8, seed=17, grad="sum", return_indices=True)
    zin = GuardBanded(n, d, ld, c0=c0, device=DEV, fill=z)
    gout = GuardBanded(n, d, ldg, c0=g0, device=DEV)
    got = triplet_loss(emb.replace(nodes=zin.window), true, hacky_cauchy_l2, relative_loss, 8, seed=17, grad="sum", return_indices=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    spec = _abi.GnfTripletSpec(_abi.GNF_TRIPLET_HACKY_CAUCHY_L2, 0.0, 0.0, 0, _abi.GNF_TRIPLET_RELATIVE, 0.0, 8, 0, 17)
    rc, outs = _raw(zin.ptr(), ld, d, true, spec, 8, gout.ptr(), ldg)
    assert rc == 0
    assert torch.equal(gout.window, want["grad_nodes"]) and bool(torch.isfinite(gout.window).all())
    assert torch.equal(outs[0], want["loss_per_node"]) and torch.equal(outs[2][0], want["sum_loss"])
    assert torch.equal(outs[4], want["pos_index"]) and torch.equal(outs[5], want["neg_index"])
    zin.check_guard()
    gout.check_guard()
    assert np.array_equal(zin.numpy(), z)


# ---- 6. more than 64 bitmap words: sparse rings on both sides of the prefix scan's chunk -------------------------------------
def test_sparse_rings_of_4096_and_4161_nodes():
    from gnf_amd.triplet_loss import l2, triplet_loss
    sizes = [4096, 4161, 3]
    s, r, o = [], [], 0
    for ng in sizes:   # a directed ring with a chord from every fourth node: one or two positives, ng - 2 or ng - 3 negatives
        i = np.arange(ng)
        s += [i + o, i[::4] + o]
        r += [(i + 1) % ng + o, (i[::4] + ng // 2) % ng + o]
        o += ng
    n_edge = [ng + len(range(0, ng, 4)) for ng in sizes]
    s, r = np.concatenate(s).astype(np.int32), np.concatenate(r).astype(np.int32)
    z = R.embeddings(sizes, 2, 0)
    true = graph_from_arrays(sizes, n_edge, s, r, np.zeros((len(z), 1), np.float32), DEV)
    draws = np.random.default_rng(3).integers(0, 2 ** 32, size=(2, 2, len(z)), dtype=np.uint64).astype(np.uint32)
    draws[0, 1, ::2], draws[0, 1, 1::2] = 2 ** 32 - 1, 0                # the last and the first unset column
    pos, neg = R.sample(sizes, s, r, draws)
    out = triplet_loss(_emb(z, sizes), true, l2, None, 2, draws=torch.as_tensor(draws.astype(np.int64)).to(DEV), grad="sum",
                       return_indices=True)
    np.testing.assert_array_equal(out["pos_index"].cpu().numpy(), pos)
    np.testing.assert_array_equal(out["neg_index"].cpu().numpy(), neg)
    assert (neg[0, 1:4096:2] < 4096).all() and neg[0, 0] == 4095 and neg[0, 4096 + 2] == 4096 + 4160 and int(out["skipped_terms"].sum()) == 0
    r64 = R.triplet_loss(z, sizes, s, r, indices=(pos, neg))
    r32 = R.triplet_loss(z, sizes, s, r, indices=(pos, neg), dtype=np.float32)
    assert R.margin_ok(r64, r32)
    _hold("rings", out, r64, r32, 2)


# ---- 7. every term of a relative loss at p + q == 0 is skipped -----------------------------------------------------------------
def test_relative_terms_with_p_plus_q_zero_are_skipped():
    from gnf_amd.triplet_loss import l2, relative_loss, triplet_loss
    sizes = R.batch()[0]
    n = int(np.sum(sizes))
    out = triplet_loss(_emb(np.zeros((n, 4), np.float32)), _true_graph(), l2, relative_loss, 3, grad="sum", return_indices=True)
    assert out["skipped_terms"].tolist() == [3 * ng for ng in sizes]
    assert bool((out["pos_index"] == -1).all()) and bool((out["neg_index"] == -1).all())
    assert float(out["sum_loss"]) == 0.0 == float(out["mean_loss"]) and not bool(out["grad_nodes"].any()) and not bool(out["loss_per_node"].any())


# ---- 8. an empty batch; invalid calls -------------------------------------------------------------------------------------------
def test_an_empty_batch_gives_zeros():
    """n_nodes == 0 with two graphs, at the entry point itself: every output is zeroed, GNF_OK"""
    from gnf_amd import _abi
    lib = _abi.lib()
    off = torch.zeros(3, dtype=torch.int32, device=DEV)
    loss = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    skipped = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    csr = _abi.GnfCsr(0, 0, 0, 0, off.data_ptr(), 2)
    spec = _abi.GnfTripletSpec(0, 0.0, 0.0, 0, 0, 0.65, 8, 0, 0)
    with torch.cuda.device(DEV):
        _abi.check(lib.gnf_triplet_loss_f32(C.byref(csr), None, 4, 4, 0, C.byref(spec), None, None, _abi.ptr(loss), _abi.ptr(sums),
                                            _abi.ptr(skipped), None, None, None, 4, 1.0, None, 0,
                                            _abi.stream_ptr(torch.device(DEV))), "gnf_triplet_loss_f32")
    torch.cuda.synchronize()
    assert loss.tolist() == [0.0, 0.0] == sums.tolist() and skipped.tolist() == [0, 0]


def test_invalid_calls_give_their_codes_with_text():
    from gnf_amd import _abi
    from gnf_amd.triplet_loss import triplet_loss
    sizes = R.batch()[0]
    z = R.embeddings(sizes, 4, 0)
    emb, true = _emb(z), _true_graph()
    zt = emb.nodes
    good = _abi.GnfTripletSpec(0, 0.0, 0.0, 0, 0, 0.65, 2, 0, 0)
    lib = _abi.lib()
    rc, _ = _raw(_abi.ptr(zt), 4, 4, true, good, 2)
    assert rc == 0
    for spec, kw, code, text in ((_abi.GnfTripletSpec(9, 0.0, 0.0, 0, 0, 0.65, 2, 0, 0), {}, -1, "score=9"),
                                 (_abi.GnfTripletSpec(0, 0.0, 0.0, 0, 0, 0.65, 65, 0, 0), {}, -2, "num_sampling_loops=65"),
                                 (good, dict(ld=3), -2, "ld=3"), (good, dict(cap=65537), -2, "max_nodes_per_graph=65537"),
                                 (good, dict(grad_ptr=_abi.ptr(zt), ldg=3), -2, "ld_grad=3")):
        args = dict(ld=4, cap=130)
        args.update(kw)
        rc, _ = _raw(_abi.ptr(zt), args["ld"], 4, true, spec, 2, args.get("grad_ptr"), args.get("ldg", 0), args["cap"])
        msg = (lib.gnf_last_error() or b"").decode()
        assert rc == code and text in msg and "gnf_triplet_loss_f32" in msg, (rc, msg)
    with pytest.raises(_abi.GnfError):
        triplet_loss(emb.to("cpu"), true)
    with pytest.raises(_abi.GnfError):
        triplet_loss(emb, true.to("cpu"))
    with pytest.raises(ValueError):
        triplet_loss(emb, true, max_nodes_per_graph=64, n_node_host=sizes)      # the largest graph has 130 nodes
    with pytest.raises(ValueError):
        triplet_loss(emb, true, max_nodes_per_graph=65537)


# ---- 9. capture ------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replayed_after_draws_are_refilled_equals_the_eager_call():
    """With max_nodes_per_graph given nothing is read back and nothing synchronises: the call is captured on one stream, the
    draws (and the embeddings) are overwritten in place, and the replay equals an eager call on the new values bit for bit."""
    from gnf_amd.triplet_loss import exp_l2, triplet_loss
    sizes = R.batch()[0]
    z = R.embeddings(sizes, 64, 0)
    n = len(z)
    emb, true = _emb(z), _true_graph()
    draws = torch.as_tensor(R.hash_draws(1, 8, n).view(np.int32)).view(torch.uint32).to(DEV)
    kw = dict(distance_fn=exp_l2, draws=draws, grad="sum", max_nodes_per_graph=130, return_indices=True)
    triplet_loss(emb, true, **kw)                        # (the first launches: CSR and offsets caches)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = triplet_loss(emb, true, **kw)
    seen = []
    for seed in (11, 12):
        draws.view(torch.int32).copy_(torch.as_tensor(R.hash_draws(seed, 8, n).view(np.int32)).to(DEV))
        emb.nodes.copy_(torch.as_tensor(R.embeddings(sizes, 64, seed)).to(DEV))
        for v in captured.values():
            v.zero_()
        cg.replay()
        torch.cuda.synchronize()
        eager = triplet_loss(emb, true, **kw)
        for k in eager:
            assert torch.equal(captured[k], eager[k]), k
        hashed = triplet_loss(emb, true, distance_fn=exp_l2, seed=seed, grad="sum", return_indices=True)
        for k in eager:
            assert torch.equal(hashed[k], eager[k]), k
        assert float(eager["sum_loss"]) > 0.0
        seen.append(captured["pos_index"].clone())
    assert not torch.equal(seen[0], seen[1])
