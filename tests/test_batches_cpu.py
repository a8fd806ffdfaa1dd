"""Batch assembly without a device (include/gnf_batches.h): header, exports and binding in step; every rejection with its code
and its text before any launch; the two statements of tests/batches_ref.py against each other (the parent route's sort
against the kernels' cut-and-rebase / arithmetic); and the chunk readers' default behaviour."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batches_ref as R
from gnf_amd import _abi, datasets as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnf_batch_assemble_workspace_bytes", "gnf_batch_assemble", "gnf_complete_batch_workspace_bytes",
               "gnf_complete_batch")
GNF_EINVAL, GNF_ESHAPE, GNF_EWORKSPACE = -1, -2, -3
P = 1 << 20   # a made-up non-null pointer: every call below fails before any launch, nothing is dereferenced


def test_symbols_are_exported_and_bound():
    main = open(os.path.join(ROOT, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_batches.h"$', main, flags=re.M)
    assert re.search(r"^#define GNF_ABI_VERSION 10$", main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "gnf_batches.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_abi.BATCH_SYMBOLS)
    for other in (_abi.EXPORTED_SYMBOLS, _abi.ORBIT_SYMBOLS, _abi.ADJ_LOSS_SYMBOLS, _abi.ENCODER_SYMBOLS, _abi.ENCODER_TRAIN_SYMBOLS,
                  _abi.DISTANCE_SYMBOLS, _abi.INVERSE_PER_GRAPH_SYMBOLS, _abi.SPECTRA_SYMBOLS, _abi.COMPONENT_SYMBOLS,
                  _abi.HASH_SYMBOLS, _abi.TRIPLET_SYMBOLS):
        assert not set(_abi.BATCH_SYMBOLS) & set(other)
    # EXPORTED_SYMBOLS still mirrors the prototypes gnf.h spells out itself
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", own))) == sorted(_abi.EXPORTED_SYMBOLS)
    lib = _abi.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
    assert lib.gnf_abi_version() == 10 == _abi.GNF_ABI_VERSION
    assert int(re.search(r"^#define GNF_BATCH_MAX_GRAPHS \(1 << (\d+)\)$", text, flags=re.M).group(1)) == 20
    assert _abi.GNF_BATCH_MAX_GRAPHS == 1 << 20
    fields = re.search(r"typedef struct GnfBatchStore \{(.*?)\}", text, flags=re.S).group(1)
    names = [n.strip(" *") for decl in re.findall(r"(?:const int32_t|const int64_t|int64_t)\s*\*?\s*([^;]+);", fields)
             for n in decl.split(",")]
    assert names == [f[0] for f in _abi.GnfBatchStore._fields_]
    flat = " ".join(raw.replace("\n * ", " ").split())
    assert "THE ARRAY IDENTITY" in flat and "no col array is written" in flat     # the header states the identity
    assert "wrong numbers, never an access outside the arrays" in flat            # ... and the clamp, in GnfCsr.node_offsets' words


def test_workspace_sizes_are_host_computations():
    lib = _abi.lib()
    a, c = lib.gnf_batch_assemble_workspace_bytes, lib.gnf_complete_batch_workspace_bytes
    assert a(0) == 8 and c(0) == 8                    # one int32 (the edge offsets' [B + 1]), rounded to 8
    assert a(9) == 9 * 8 + 10 * 4 + 9 * 4 + 4 and c(9) == 40
    assert a(-1) == 0 and c(-1) == 0 and a((1 << 20) + 1) == 0 and c((1 << 20) + 1) == 0 and a(1 << 20) > 0 and c(1 << 20) > 0
    for lo, hi in ((0, 1), (7, 300), (4095, 4096)):
        assert a(lo) <= a(hi) and c(lo) <= c(hi)


def _assemble(store=True, ids=P, b=4, n=10, e=20, outs=None, ws=P, ws_bytes=None, store_sizes=(10, 100, 1000), store_ptrs=None):
    lib = _abi.lib()
    st = _abi.GnfBatchStore(*(store_ptrs or (P,) * 8), *store_sizes)
    outs = [P] * 9 if outs is None else outs
    ws_bytes = max(lib.gnf_batch_assemble_workspace_bytes(b), 8) if ws_bytes is None else ws_bytes
    rc = lib.gnf_batch_assemble(C.byref(st) if store else None, ids, b, n, e, *outs, ws, ws_bytes, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def _complete(n_node=P, b=4, n=10, e=30, outs=None, ws=P, ws_bytes=None):
    lib = _abi.lib()
    outs = [P] * 5 if outs is None else outs
    ws_bytes = max(lib.gnf_complete_batch_workspace_bytes(b), 8) if ws_bytes is None else ws_bytes
    rc = lib.gnf_complete_batch(n_node, b, n, e, *outs, ws, ws_bytes, None)
    return rc, (lib.gnf_last_error() or b"").decode()


def _none_at(k, count):
    return [None if i == k else P for i in range(count)]


def test_batch_assemble_rejections_come_with_their_code_and_text():
    bad = [(dict(store=False), GNF_EINVAL), (dict(ids=None), GNF_EINVAL), (dict(ws=None), GNF_EINVAL)]
    bad += [(dict(outs=_none_at(k, 9)), GNF_EINVAL) for k in range(9)]
    bad += [(dict(store_ptrs=_none_at(k, 8)), GNF_EINVAL) for k in range(8)]
    bad += [(dict(b=-1), GNF_ESHAPE), (dict(n=-1), GNF_ESHAPE), (dict(e=-1), GNF_ESHAPE), (dict(b=(1 << 20) + 1), GNF_ESHAPE),
            (dict(e=2 ** 31), GNF_ESHAPE), (dict(n=2 ** 31), GNF_ESHAPE), (dict(store_sizes=(-1, 100, 1000)), GNF_ESHAPE),
            (dict(store_sizes=(10, 100, 2 ** 31)), GNF_ESHAPE), (dict(store_sizes=(0, 0, 0)), GNF_ESHAPE),
            (dict(ws_bytes=_abi.lib().gnf_batch_assemble_workspace_bytes(4) - 1), GNF_EWORKSPACE), (dict(ws_bytes=0), GNF_EWORKSPACE)]
    for kw, code in bad:
        rc, msg = _assemble(**kw)
        assert rc == code and msg.startswith("gnf_batch_assemble"), (kw, rc, msg)
    assert "workspace" in _assemble(ws_bytes=0)[1] and "null" in _assemble(ids=None)[1] and "n_batch=-1" in _assemble(b=-1)[1]


def test_complete_batch_rejections_come_with_their_code_and_text():
    bad = [(dict(n_node=None), GNF_EINVAL), (dict(ws=None), GNF_EINVAL)]
    bad += [(dict(outs=_none_at(k, 5)), GNF_EINVAL) for k in range(5)]
    bad += [(dict(b=-1), GNF_ESHAPE), (dict(n=-1), GNF_ESHAPE), (dict(e=-1), GNF_ESHAPE), (dict(b=(1 << 20) + 1), GNF_ESHAPE),
            (dict(n=46341, e=46341 ** 2), GNF_ESHAPE),          # sum n_g^2 > INT32_MAX: rowptr is int32
            (dict(ws_bytes=_abi.lib().gnf_complete_batch_workspace_bytes(4) - 1), GNF_EWORKSPACE)]
    for kw, code in bad:
        rc, msg = _complete(**kw)
        assert rc == code and msg.startswith("gnf_complete_batch"), (kw, rc, msg)
    assert 46341 ** 2 > 2 ** 31 - 1 >= 46340 ** 2


def test_python_entry_points_need_a_device_and_check_their_arguments():
    with pytest.raises(_abi.GnfError):
        D.DeviceGraphDataset(R.dataset(), 4, device="cpu")
    with pytest.raises(_abi.GnfError):
        D.complete_batch(np.zeros((3, 2), np.float32), [1, 2], "cpu")


# ---- the reference checks itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [R.COMPLETE_SIZES, R.COMPLETE_GRID, []], ids=["mixed", "grid361", "empty"])
def test_complete_closed_form_is_senders_receivers_and_both_csrs(sizes):
    want, col, rowptr_t, col_t = R.complete_host_route(sizes)
    got = R.complete_closed_form(sizes)
    assert sorted(got) == sorted(R.COMPLETE_KEYS)
    for k in R.COMPLETE_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    # the array identity: by-receiver col == by-sender col == receivers, and the two rowptrs are one array
    assert np.array_equal(col, want["receivers"]) and np.array_equal(col_t, want["receivers"])
    assert np.array_equal(rowptr_t, want["rowptr"])
    n = np.asarray(sizes, np.int64)
    assert np.array_equal(want["rowptr"], np.concatenate([[0], np.cumsum(np.repeat(n, n))]))


@pytest.mark.parametrize("name", ["empty", "one", "mixed", "reversed", "drawn64"])
def test_cut_and_rebase_is_the_csr_of_the_assembled_batch(name):
    ds = R.dataset()
    ids = R.id_lists(ds)[name]
    want, got = R.host_route(ds, ids), R.cut_and_rebase(ds, ids)
    assert sorted(got) == sorted(R.ASSEMBLE_KEYS)
    for k in R.ASSEMBLE_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert len(want["senders"]) == int(ds.n_edge[ids].sum()) if len(ids) else len(want["senders"]) == 0


def test_the_dataset_has_what_the_cases_are_there_for():
    ds = R.dataset()
    assert sorted(ds.n_node.tolist()) == sorted([1, 2, 17, 64, 65, 33, 5, 4, 3, 65])
    assert R.id_lists(ds)["mixed"] == [3, 3, 0, 6, 5, 1, 4, 2, 3] and {R.COMPLETE, R.EDGELESS, R.LOOP_ONLY} <= set(R.IDS_MIXED)
    n, s, r = ds.graph(R.LOOP_ONLY)
    assert n == 3 and s.tolist() == r.tolist() == [1]
    multi = 0
    for g in range(len(ds)):
        n, s, r = ds.graph(g)
        pairs = s.astype(np.int64) * n + r
        multi += len(pairs) - len(np.unique(pairs))
        if g not in (R.COMPLETE, R.EDGELESS, R.LOOP_ONLY) and n > 2:
            und = set(zip(s.tolist(), r.tolist()))
            assert any((b, a) not in und for a, b in und)                       # directed
    assert multi >= 10
    assert ds.n_edge[R.COMPLETE] > 4 * 1024                                     # more words than four fill workgroups' worth
    assert len(set(R.id_lists(ds)["drawn64"])) < 64


# ---- chunk readers: device=None is the behaviour there was ---------------------------------------------------------------------
def _write_chunks(path, rng, files=2, graphs=7, dim=3):
    chunks = []
    for k in range(files):
        n_node = rng.integers(2, 9, size=graphs).astype(np.int32)
        emb = rng.standard_normal((int(n_node.sum()), dim))
        D.write_embedding_chunk(os.path.join(path, f"chunk_{k}.pkl"), emb, n_node)
        chunks.append((emb, n_node))
    return chunks


def test_chunk_readers_without_a_device_hand_out_what_they_did(tmp_path):
    chunks = _write_chunks(str(tmp_path), np.random.default_rng(5))
    fixed = D.GrevnetDatasetFixed(str(tmp_path), 3, sort_files=True)
    variable = D.GrevnetDatasetVariable(str(tmp_path), 20, sort_files=True)
    assert fixed.device is None and variable.device is None
    for data, plan in ((fixed, lambda nn: D.plan_fixed_batches(nn, 3)), (variable, lambda nn: D.plan_variable_batches(nn, 20))):
        for emb, n_node in chunks:
            row_end = np.concatenate([[0], np.cumsum(n_node)])
            for lo, hi in plan(n_node):
                z, nn = data.train_batch()
                assert isinstance(z, np.ndarray) and z.dtype == emb.dtype and isinstance(nn, np.ndarray)
                assert np.array_equal(z, emb[row_end[lo]:row_end[hi]]) and np.array_equal(nn, n_node[lo:hi])
        with pytest.raises(IndexError):
            data.train_batch()
