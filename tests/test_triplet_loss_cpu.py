"""The sampled triplet loss without a device: the restatement of tests/triplet_loss_ref.py against a literal dense form of
loss.py:221-270, the hash that replaces TF's random stream, the seed condition of the GPU tests, tokens, argument errors, the
binding and the example's flags."""
import importlib.util
import os
import re

import numpy as np
import pytest

import triplet_loss_ref as R
from gnf_amd import _abi
from helpers import graph_from_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnf_triplet_loss_workspace_bytes", "gnf_triplet_loss_f32")
ALL_SCORES = [R.L2, R.DOT, R.EXP_L2, R.HACKY, R.SCALED_HACKY, R.sigmoid_l2(3.0, 2.0), R.CAUCHY, R.SIGMOID_DOT]


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [R.MARGIN, R.RELATIVE], ids=["margin", "relative"])
@pytest.mark.parametrize("score", ALL_SCORES, ids=lambda s: "-".join(str(v) for v in s))
def test_restatement_against_the_literal_dense_form(score, loss):
    sizes, _, s, r = R.batch()
    z = R.embeddings(sizes, 7, 3)
    ref = R.triplet_loss(z, sizes, s, r, score, loss, loops=4, seed=11)
    literal, true_adj, inv = R.triplet_loss_literal(z, sizes, s, r, score, loss, ref["pos"], ref["neg"])
    rows = np.arange(len(z))
    for l in range(4):   # every chosen index has weight in the matrix the reference samples from
        ok = ref["pos"][l] >= 0
        assert (true_adj[rows[ok], ref["pos"][l, ok]] > 0).all() and (inv[rows[ok], ref["neg"][l, ok]] == 1).all()
    scale = max(1.0, float(np.abs(literal).max()))
    assert np.abs(literal - ref["loss_per_node"]).max() <= 1e-9 * scale   # (r - 2 z z^T + r^T against sum (z_i - z_j)^2)
    assert ref["loss_per_node"].sum() == pytest.approx(ref["sum_loss"], rel=1e-12)
    assert ref["loss_per_graph"].sum() == pytest.approx(ref["sum_loss"], rel=1e-12)
    kept = len(z) * 4 - int(ref["skipped"].sum())
    assert ref["mean_loss"] == pytest.approx(ref["sum_loss"] / kept, rel=1e-12)


def test_candidates_follow_the_reference_matrices():
    """positives: the row of true_adj with multiplicity, a self loop included; negatives: the row of inv_true_adj"""
    sizes, _, s, r = R.batch()
    n = int(np.sum(sizes))
    _, true_adj, inv = R.triplet_loss_literal(np.zeros((n, 1)), sizes, s, r, R.L2, R.MARGIN, np.zeros((0, n), np.int32),
                                              np.zeros((0, n), np.int32))
    doubled = loops = 0
    for i, (pos, neg) in enumerate(R.candidates(sizes, s, r)):
        assert np.array_equal(np.bincount(pos, minlength=n), true_adj[i].astype(np.int64))
        assert neg == np.flatnonzero(inv[i] > 0).tolist()       # (1 - true_adj is -1 at a duplicated edge: no candidate)
        doubled += len(pos) != len(set(pos))
        loops += i in pos
    assert doubled >= 3 and 50 < loops < n - 50                 # duplicated edges; self loops on about half the nodes
    for i, (pos, neg) in enumerate(R.candidates(sizes, s, r, "skip")):
        assert i not in pos and i not in neg
    o = int(np.sum(R.SIZES))
    cand = R.candidates(sizes, s, r)
    assert all(len(cand[i][0]) == R.COMPLETE - 1 and not cand[i][1] for i in range(o, o + R.COMPLETE))      # no negatives
    assert all(not cand[i][0] and len(cand[i][1]) == R.EDGELESS - 1 for i in range(o + R.COMPLETE, n))       # no positives
    # sample() walks no list of negatives: the same choices as indexing the lists
    draws = np.random.default_rng(1).integers(0, 2 ** 32, size=(3, 2, n), dtype=np.uint64).astype(np.uint32)
    draws[0, :, :40], draws[1, :, :40] = 0, 2 ** 32 - 1                                     # the first and the last candidate
    for mode in ("keep", "skip"):
        pos, neg = R.sample(sizes, s, r, draws, mode)
        for i, (cp, cn) in enumerate(R.candidates(sizes, s, r, mode)):
            for l in range(3):
                want = (cp[R.choose(draws[l, 0, i], len(cp))], cn[R.choose(draws[l, 1, i], len(cn))]) if cp and cn else (-1, -1)
                assert (pos[l, i], neg[l, i]) == want, (mode, i, l)


def test_skipped_terms():
    """nodes without a candidate: index -1, term 0, no gradient, counted per graph; so is a relative term with p + q == 0"""
    sizes, _, s, r = R.batch()
    z = R.embeddings(sizes, 3, 0)
    ref = R.triplet_loss(z, sizes, s, r, R.L2, R.MARGIN, loops=2, seed=5)
    cand = R.candidates(sizes, s, r)
    none = np.asarray([not (p and q) for p, q in cand])
    assert none.sum() >= R.COMPLETE + R.EDGELESS + 1 and ((ref["pos"] < 0) == none[None]).all() and ((ref["neg"] < 0) == none[None]).all()
    assert not ref["loss_per_node"][none].any()
    assert ref["skipped"][-2:].tolist() == [2 * R.COMPLETE, 2 * R.EDGELESS] and ref["skipped"][0] == 2   # (a 1-node graph)
    assert not ref["grad"][-R.EDGELESS:].any() and not ref["grad"][-R.EDGELESS - R.COMPLETE:-R.EDGELESS].any()
    zero = R.triplet_loss(np.zeros_like(z), sizes, s, r, R.L2, R.RELATIVE, loops=2, seed=5)
    assert (zero["pos"] < 0).all() and zero["sum_loss"] == 0.0 == zero["mean_loss"] and not zero["grad"].any()
    assert zero["skipped"].tolist() == [2 * ng for ng in sizes]


@pytest.mark.parametrize("loss", [R.MARGIN, R.RELATIVE], ids=["margin", "relative"])
@pytest.mark.parametrize("score", ALL_SCORES, ids=lambda s: "-".join(str(v) for v in s))
def test_closed_form_gradient_against_central_differences(score, loss):
    sizes, s, r = [6, 9], *R.AL.true_graph([6, 9], 2)[1:]
    z = R.embeddings(sizes, 3, 4).astype(np.float64)
    ref = R.triplet_loss(z, sizes, s, r, score, loss, loops=8, seed=3)
    idx = (ref["pos"], ref["neg"])
    assert np.abs(ref["grad"]).max() > 1e-3
    assert (np.isnan(ref["kink"]) | (np.abs(ref["kink"]) > (1e-4 if loss[0] == "margin" else 0.0))).all()   # no hinge at its kink
    h = 1e-6
    for k in range(z.shape[0]):
        for f in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[k, f] += h
            zm[k, f] -= h
            fd = (R.triplet_loss(zp, sizes, s, r, score, loss, indices=idx)["sum_loss"]
                  - R.triplet_loss(zm, sizes, s, r, score, loss, indices=idx)["sum_loss"]) / (2 * h)
            assert abs(fd - ref["grad"][k, f]) <= 1e-6 * max(1.0, np.abs(ref["grad"]).max()), (k, f, fd, ref["grad"][k, f])


# ---- the hash --------------------------------------------------------------------------------------------------------------
def test_hash_is_uniform_over_the_candidates():
    """five nodes, both draw kinds, cnt in {2, 3, 7}, 16 seeds x 64 rounds = 1024 draws each: every bin within 5 sigma"""
    worst = 0.0
    for i in range(5):
        for which in (0, 1):
            draws = [R.hash_draw(seed, l, which, i) for seed in range(16) for l in range(64)]
            for cnt in (2, 3, 7):
                bins = np.bincount([R.choose(x, cnt) for x in draws], minlength=cnt)
                assert len(bins) == cnt
                sigma = np.sqrt(1024.0 * (1.0 / cnt) * (1.0 - 1.0 / cnt))
                dev = float(np.abs(bins - 1024.0 / cnt).max() / sigma)
                worst = max(worst, dev)
                assert dev <= 5.0, (i, which, cnt, bins)
    print(f"hash: largest deviation {worst:.2f} sigma")


def test_hash_values_and_the_candidate_rule():
    assert all(0 <= R.hash_draw(s, l, w, i) < 2 ** 32 for s in (0, 2 ** 64 - 1) for l in (0, 63) for w in (0, 1) for i in (0, 2 ** 31 - 2))
    assert len({R.hash_draw(0, l, w, i) for l in range(8) for w in (0, 1) for i in range(64)}) == 1024
    assert R.choose(0, 7) == 0 and R.choose(2 ** 32 - 1, 7) == 6 and R.choose(2 ** 31, 2) == 1 and R.choose(2 ** 31 - 1, 2) == 0
    d = R.hash_draws(9, 3, 5)
    assert d.dtype == np.uint32 and d.shape == (3, 2, 5) and int(d[2, 1, 4]) == R.hash_draw(9, 2, 1, 4)


# ---- the seed condition of the GPU tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [R.MARGIN, R.RELATIVE], ids=["margin", "relative"])
@pytest.mark.parametrize("name", list(R.SCORES))
def test_a_seed_with_margin_exists(name, loss):
    for d, loops, self_loops in ((1, 8, "keep"), (64, 1, "skip"), (257, 8, "keep")):
        seed, z, r64, r32 = R.pick_seed(d, R.SCORES[name], loss, loops, self_loops)
        assert seed is not None, (d, loops, self_loops)
        assert np.array_equal(r64["pos"], r32["pos"]) and np.array_equal(r64["neg"], r32["neg"])
        assert all(v > 0 for v in R.bounds(r64, r32).values())


def test_margin_condition_rejects_a_term_on_the_kink():
    sizes, s, r = [4], np.asarray([0, 1, 2, 3], np.int32), np.asarray([1, 2, 3, 0], np.int32)
    z = np.zeros((4, 2), np.float32)
    z[:, 0] = [0.0, 1.0, 2.0, 3.0]
    idx = (np.asarray([[1, 2, 3, 0]], np.int32), np.asarray([[2, 3, 0, 1]], np.int32))   # node 0: p = 1, q = 4; node 1: 1, 4 ...
    on = (R.triplet_loss(z, sizes, s, r, R.L2, ("margin", -3.0), indices=idx), R.triplet_loss(z, sizes, s, r, R.L2, ("margin", -3.0), indices=idx, dtype=np.float32))
    off = (R.triplet_loss(z, sizes, s, r, R.L2, ("margin", -2.5), indices=idx), R.triplet_loss(z, sizes, s, r, R.L2, ("margin", -2.5), indices=idx, dtype=np.float32))
    assert on[0]["kink"][0, 0] == 0.0 and R.margin_ok(*on)          # exactly on it in both precisions: the same side in both
    assert R.margin_ok(*off)
    near = dict(off[1], kink=off[1]["kink"] * 1e-9)
    assert not R.margin_ok(off[0], near)


# ---- tokens, arguments, binding --------------------------------------------------------------------------------------------
def _cpu_graphs():
    sizes, n_edge, s, r = R.batch()
    z = R.embeddings(sizes, 3, 0)
    none = np.zeros(0, np.int32)
    return (graph_from_arrays(sizes, np.zeros(len(sizes), np.int32), none, none, z, "cpu"),
            graph_from_arrays(sizes, n_edge, s, r, np.zeros((len(z), 1), np.float32), "cpu"))


def test_tokens():
    import torch
    from gnf_amd import adj_loss, triplet_loss as fn
    from gnf_amd.flow import scaled_hacky_sigmoid_l2
    T = importlib.import_module("gnf_amd.triplet_loss")          # (gnf_amd.triplet_loss, the attribute, is the function)
    assert fn is T.triplet_loss
    kinds = [T.score_params(t)[0] for t in (T.l2, T.dot, T.exp_l2, T.hacky_cauchy_l2, T.sigmoid_dot)]
    assert kinds == [_abi.GNF_TRIPLET_L2, _abi.GNF_TRIPLET_DOT, _abi.GNF_TRIPLET_EXP_L2, _abi.GNF_TRIPLET_HACKY_CAUCHY_L2,
                     _abi.GNF_TRIPLET_SIGMOID_DOT]
    assert T.score_params(scaled_hacky_sigmoid_l2) == (_abi.GNF_TRIPLET_SIGMOID_L2, 10.0, 1.0, 1)
    assert T.score_params(adj_loss.hacky_sigmoid_l2) == (_abi.GNF_TRIPLET_SIGMOID_L2, 10.0, 1.0, 0)
    assert T.score_params(adj_loss.sigmoid_l2(3.0, 2.0)) == (_abi.GNF_TRIPLET_SIGMOID_L2, 3.0, 2.0, 1)
    assert T.loss_params(T.margin_loss()) == (_abi.GNF_TRIPLET_MARGIN, 0.65) and T.loss_params(T.margin_loss(0.25))[1] == 0.25
    assert T.loss_params(T.margin_loss) == (_abi.GNF_TRIPLET_MARGIN, 0.65) and T.loss_params(T.relative_loss)[0] == _abi.GNF_TRIPLET_RELATIVE
    for bad in (adj_loss.TunedSigmoidL2(), torch.sigmoid, "l2", None, [1]):
        with pytest.raises(NotImplementedError):
            T.score_params(bad)
    for bad in (T.l2, "margin", None, max):
        with pytest.raises(NotImplementedError):
            T.loss_params(bad)
    for token in (T.l2, T.dot, T.exp_l2, T.hacky_cauchy_l2, T.sigmoid_dot, T.relative_loss):
        with pytest.raises(NotImplementedError):
            token(np.zeros((2, 2)))
    from gnf_amd import encoder
    with pytest.raises(Exception):          # the new tokens are not the decoder's: encoder.distance_of keeps refusing them
        encoder.distance_of({"distance": {"kind": "exp_l2"}})


def test_argument_errors_and_cpu_tensors_raise():
    import torch
    from gnf_amd import adj_loss
    T = importlib.import_module("gnf_amd.triplet_loss")
    emb, true = _cpu_graphs()
    with pytest.raises(_abi.GnfError):
        T.triplet_loss(emb, true)
    with pytest.raises(_abi.GnfError):
        T.triplet_loss(emb, true, distance_fn=T.exp_l2, triplet_loss_fn=T.relative_loss, grad="sum", return_indices=True)
    with pytest.raises(NotImplementedError):
        T.triplet_loss(emb, true, distance_fn=torch.sigmoid)
    with pytest.raises(NotImplementedError):
        T.triplet_loss(emb, true, distance_fn=adj_loss.TunedSigmoidL2())
    with pytest.raises(NotImplementedError):
        T.triplet_loss(emb, true, triplet_loss_fn=T.l2)
    for kw in (dict(grad="both"), dict(self_loops="drop"), dict(num_sampling_loops=0), dict(num_sampling_loops=65)):
        with pytest.raises(ValueError):
            T.triplet_loss(emb, true, **kw)
    with pytest.raises(ValueError):
        T.triplet_loss(emb, true.replace(nodes=true.nodes[:-1]))


def test_trainer_arguments():
    from gnf_amd import adj_loss, encoder
    from gnf_amd.train import EncoderTrainer
    T = importlib.import_module("gnf_amd.triplet_loss")
    enc = encoder.make_encoder(dict(node_dim=4, latent=8, K=1, activation="leaky_relu", num_timesteps=1, agg="mean", combine="agg",
                                    epsilon=2.0))
    tr = EncoderTrainer(enc)
    assert tr.loss_type == "binary" and EncoderTrainer.LOSS_TYPES == ("binary", "triplet")
    tr = EncoderTrainer(enc, loss_type="triplet")
    assert tr.triplet_dist_fn is T.l2 and tr.triplet_adj_dist_fn is adj_loss.hacky_sigmoid_l2 and tr.num_sampling_loops == 8
    assert isinstance(tr.triplet_loss_fn, T.margin_loss) and tr.triplet_loss_fn.margin == 0.65 and tr.seed == 0 and tr.draws is None
    with pytest.raises(ValueError):
        EncoderTrainer(enc, loss_type="triplet", tune_sigmoid=True, distance_fn=adj_loss.sigmoid_l2(10.0, 1.0))
    with pytest.raises(ValueError):
        EncoderTrainer(enc, loss_type="hinge")
    with pytest.raises(ValueError):
        EncoderTrainer(enc, loss_type="triplet", num_sampling_loops=65)
    with pytest.raises(NotImplementedError):
        EncoderTrainer(enc, loss_type="triplet", triplet_dist_fn=max)
    with pytest.raises(NotImplementedError):
        EncoderTrainer(enc, loss_type="triplet", triplet_adj_dist_fn=T.exp_l2)
    with pytest.raises(NotImplementedError):
        EncoderTrainer(enc, loss_type="triplet", triplet_adj_dist_fn=adj_loss.TunedSigmoidL2())


def test_symbols_are_exported_and_bound():
    """include/gnf_triplet_loss.h (included by gnf.h), the library's exports and _abi.TRIPLET_SYMBOLS are in step"""
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_triplet_loss.h"$', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_triplet_loss.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.TRIPLET_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS, _abi.ENCODER_TRAIN_SYMBOLS,
                  _abi.DISTANCE_SYMBOLS, _abi.INVERSE_PER_GRAPH_SYMBOLS, _abi.SPECTRA_SYMBOLS, _abi.COMPONENT_SYMBOLS,
                  _abi.HASH_SYMBOLS):
        assert not set(_abi.TRIPLET_SYMBOLS) & set(other)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    enums = dict(re.findall(r"\b(GNF_TRIPLET_[A-Z0-9_]+) = (\d+)", text))
    assert len(enums) == 10 and all(getattr(_abi, k) == int(v) for k, v in enums.items())
    T = importlib.import_module("gnf_amd.triplet_loss")
    defines = {k: int(v) for k, v in re.findall(r"^#define GNF_TRIPLET_(\w+) (\d+)$", text, flags=re.M)}
    assert defines == {"MAX_LOOPS": T.MAX_SAMPLING_LOOPS, "MAX_NODES": T.MAX_NODES_PER_GRAPH}
    fields = re.search(r"typedef struct GnfTripletSpec \{(.*?)\}", text, flags=re.S).group(1)
    names = [n for decl in re.findall(r"(?:int32_t|float|uint64_t) ([^;]+);", fields) for n in re.split(r",\s*", decl)]
    assert names == [f[0] for f in _abi.GnfTripletSpec._fields_]
    src = open(os.path.join(ROOT, "graph-normalizing-flows_amd", "csrc", "gnf_triplet_loss.hip")).read()
    for k in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB):   # the hash, as the header and the kernel spell it
        assert f"0x{k:X}" in raw and f"0x{k:X}ull" in src


def test_workspace_size_is_a_host_computation():
    ws = _abi.lib().gnf_triplet_loss_workspace_bytes
    # three int32 / fp32 arrays of [N][2 L], the rows' fp64 sums, four int32 per row
    assert ws(3, 100, 8) == 3 * 100 * 16 * 4 + 100 * 8 + 4 * 100 * 4
    assert ws(1, 7, 1) == (3 * 7 * 2 * 4 + 7 * 8 + 4 * 7 * 4 + 7) // 8 * 8 and ws(0, 0, 1) == 0
    assert ws(-1, 10, 8) == 0 and ws(1, -1, 8) == 0 and ws(1, 10, 0) == 0 and ws(1, 10, 65) == 0
    assert ws(1, 2 ** 24, 64) == 0 and ws(1, 2 ** 24 - 1, 64) > 0        # N * 2 L has to fit int32
    for a, b in ((0, 1), (7, 300), (4095, 4096)):
        assert ws(3, a, 8) <= ws(3, b, 8)


def _null_call(csr=None, spec=None, **kw):
    """gnf_triplet_loss_f32 on made-up pointers: every check below fails before any launch (no device is touched)"""
    import ctypes as C
    P = 1 << 20
    a = dict(z=P, ld=4, d=4, cap=20, draws=None, node=P, graph=P, sums=P, skipped=P, pos=None, neg=None, grad=None, ldg=4, ws=P,
             ws_bytes=1 << 30)
    a.update(kw)
    csr = _abi.GnfCsr(P, P, 40, 100, P, 3) if csr is None else csr
    spec = _abi.GnfTripletSpec(0, 0.0, 0.0, 0, 0, 0.65, 8, 0, 0) if spec is None else spec
    lib = _abi.lib()
    rc = lib.gnf_triplet_loss_f32(C.byref(csr) if csr else None, a["z"], a["ld"], a["d"], a["cap"], C.byref(spec) if spec else None,
                                  a["draws"], a["node"], a["graph"], a["sums"], a["skipped"], a["pos"], a["neg"], a["grad"],
                                  a["ldg"], 1.0, a["ws"], a["ws_bytes"], None)
    return rc, (lib.gnf_last_error() or b"").decode()


def test_invalid_calls_give_their_codes_before_any_launch():
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
    P = 1 << 20
    spec = lambda **kw: _abi.GnfTripletSpec(**dict(dict(score=0, loss=0, margin=0.65, num_sampling_loops=8), **kw))
    cases = [
        (dict(csr=False), EINVAL, "null csr_t"), (dict(spec=False), EINVAL, "null spec"),
        (dict(spec=spec(score=6)), EINVAL, "score=6"), (dict(spec=spec(loss=2)), EINVAL, "loss=2"),
        (dict(spec=spec(self_loops=2)), EINVAL, "self_loops=2"),
        (dict(d=0), ESHAPE, "D=0"), (dict(ld=3), ESHAPE, "ld=3"), (dict(grad=P, ldg=3), ESHAPE, "ld_grad=3"),
        (dict(spec=spec(num_sampling_loops=0)), ESHAPE, "num_sampling_loops=0"),
        (dict(spec=spec(num_sampling_loops=65)), ESHAPE, "num_sampling_loops=65"),
        (dict(cap=-1), ESHAPE, "max_nodes_per_graph=-1"), (dict(cap=65537), ESHAPE, "max_nodes_per_graph=65537"),
        (dict(cap=0), ESHAPE, "max_nodes_per_graph=0"),
        (dict(csr=_abi.GnfCsr(P, P, -1, 0, P, 3)), ESHAPE, "n_nodes=-1"),
        (dict(csr=_abi.GnfCsr(P, P, 2 ** 28, 0, P, 3)), ESHAPE, "INT32_MAX"),
        (dict(csr=_abi.GnfCsr(P, P, 40, 100, None, 3)), EINVAL, "node_offsets"),
        (dict(csr=_abi.GnfCsr(None, P, 40, 100, P, 3)), EINVAL, "null pointer"),
        (dict(csr=_abi.GnfCsr(P, None, 40, 100, P, 3)), EINVAL, "null pointer"),
        (dict(z=None), EINVAL, "null pointer"), (dict(sums=None), EINVAL, "null pointer"), (dict(node=None), EINVAL, "null pointer"),
        (dict(graph=None), EINVAL, "null pointer"), (dict(skipped=None), EINVAL, "null pointer"), (dict(ws=None), EINVAL, "null pointer"),
        (dict(ws_bytes=_abi.lib().gnf_triplet_loss_workspace_bytes(3, 40, 8) - 1), EWORKSPACE, "workspace"),
    ]
    for kw, code, text in cases:
        rc, msg = _null_call(**kw)
        assert rc == code and text in msg and "gnf_triplet_loss_f32" in msg, (kw, rc, msg)


# ---- the example -----------------------------------------------------------------------------------------------------------
def test_the_example_parses_the_reference_flags():
    spec = importlib.util.spec_from_file_location("run_gnn_example", os.path.join(ROOT, "examples", "run_gnn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    F = mod.make_parser().parse_args([])
    assert (F.loss_type, F.triplet_dist_fn, F.triplet_adj_dist_fn, F.triplet_loss_fn, F.num_sampling_loops) == \
        ("binary", "l2", "hacky_sigmoid_l2", "margin", 8)                               # run_gnn.py:82-91
    F = mod.make_parser().parse_args(["--loss_type", "triplet", "--triplet_dist_fn", "exp_l2", "--triplet_adj_dist_fn",
                                      "scaled_hacky_sigmoid_l2", "--triplet_loss_fn", "relative", "--num_sampling_loops", "3"])
    assert (F.loss_type, F.triplet_dist_fn, F.triplet_loss_fn, F.num_sampling_loops) == ("triplet", "exp_l2", "relative", 3)
    assert set(mod.TRIPLET_DIST_FNS) == {"l2", "dot", "exp_l2", "hacky_cauchy_l2", "sigmoid_dot", "scaled_hacky_sigmoid_l2",
                                         "hacky_sigmoid_l2", "sigmoid_l2"}               # DIST_FN_MAP of run_gnn.py:155-164
    assert set(mod.TRIPLET_LOSS_FNS) == {"margin", "relative"} and mod.TRIPLET_LOSS_FNS["margin"].margin == 0.65
    for bad in (["--loss_type", "hinge"], ["--triplet_dist_fn", "cosine"], ["--triplet_adj_dist_fn", "l2"], ["--triplet_loss_fn", "x"]):
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(bad)
