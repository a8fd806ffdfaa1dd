#!/usr/bin/env python3
"""Record the bits of the decoders' and the adjacency loss's old entry points, on the device.

    python tests/golden/make_pair_family_digests.py        # -> tests/golden/pair_family_digests.json

Raw ctypes calls to gnf_pred_adj_f32, gnf_adj_edges_count_f32 + gnf_adj_edges_fill (thresholds 0.1 / 0.5 / 0.9) and
gnf_adj_loss_f32 with a gradient, on the 198 nodes of adj_loss_ref.SIZES with duplicated rows, at D = 7, 200, 400, 1030 (one
per instance of the pair kernel, both routes of the decode kernels); the loss over (10, 1, scaled), (10, 1, unscaled) and
(3, 2, scaled), hard and soft labels.  Every output buffer's raw bytes go through sha256: a refactor of these files must
reproduce every bit, and tests/test_pair_family_bits_gpu.py holds the library to the file.  The loss's workspace is followed by
a guard band that the call must leave alone.

The digests pin the toolchain's expf / log1pf as much as the kernels: after a ROCm upgrade re-record them ON PURPOSE, from a
build of the commit named in the file (GNF_LIB_PATH selects a library built from another checkout, GNF_DIGESTS_COMMIT names it).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "pair_family_digests.json")

DIMS = [7, 200, 400, 1030]
THRESHOLDS = [0.1, 0.5, 0.9]
SPECS = {"10_1_scaled": (10.0, 1.0, 1), "10_1_unscaled": (10.0, 1.0, 0), "3_2_scaled": (3.0, 2.0, 1)}
SEED = 5
GUARD = 4096
DEV = "cuda:0"


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def measure():
    """{case: sha256 of the outputs' bytes} from the library gnf_amd._abi loads"""
    import numpy as np
    import torch
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    from helpers import graph_from_arrays
    import adj_loss_ref as R
    lib, st = _abi.lib(), _abi.stream_ptr(torch.device(DEV))
    sizes = R.SIZES
    b, n, cap = len(sizes), int(sum(sizes)), max(sizes)
    n_edge, s, r = R.true_graph(sizes, SEED)
    true = graph_from_arrays(sizes, n_edge, s, r, np.zeros((n, 1), np.float32), DEV)
    desc = csr_desc(true, csr_of(true), node_offsets=True)
    nn = true.n_node.to(torch.int32).contiguous()
    out = {}
    for d in DIMS:
        z = torch.as_tensor(R.embeddings(sizes, d, SEED, duplicate_rows=True)).to(DEV)
        # pred_adj
        blocks = torch.full((sum(k * k for k in sizes),), -1.0, dtype=torch.float32, device=DEV)
        off = torch.empty(b + 1, dtype=torch.int64, device=DEV)
        ws_bytes = lib.gnf_pred_adj_workspace_bytes(b)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        _abi.check(lib.gnf_pred_adj_f32(_abi.ptr(z), z.stride(0), d, _abi.ptr(nn), b, cap, _abi.ptr(blocks), _abi.ptr(off),
                                        _abi.ptr(ws), ws_bytes, st), "gnf_pred_adj_f32")
        out[f"pred_adj/D{d}"] = _sha(blocks, off)
        # edge lists
        for thr in THRESHOLDS:
            rowptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
            ne = torch.empty(b, dtype=torch.int32, device=DEV)
            total = torch.empty(1, dtype=torch.int64, device=DEV)
            ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, cap)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
            _abi.check(lib.gnf_adj_edges_count_f32(_abi.ptr(z), z.stride(0), d, _abi.ptr(nn), b, n, cap, thr, 0, _abi.ptr(rowptr),
                                                   _abi.ptr(ne), _abi.ptr(total), _abi.ptr(ws), ws_bytes, st),
                       "gnf_adj_edges_count_f32")
            e = int(total.item())
            es = torch.full((e,), -1, dtype=torch.int32, device=DEV)
            er = torch.full((e,), -1, dtype=torch.int32, device=DEV)
            _abi.check(lib.gnf_adj_edges_fill(b, n, cap, _abi.ptr(rowptr), e, _abi.ptr(es), _abi.ptr(er), _abi.ptr(ws), ws_bytes,
                                              st), "gnf_adj_edges_fill")
            out[f"edges/D{d}/thr{thr}"] = _sha(rowptr, ne, total, es, er)
        # the loss with its gradient
        for name, (temp, shift, scaled) in SPECS.items():
            for soft in (0, 1):
                spec = _abi.GnfAdjLossSpec(temp, shift, scaled, soft, 0.1, 0.5)
                sums2 = torch.empty(2, dtype=torch.float64, device=DEV)
                loss = torch.empty(b, dtype=torch.float64, device=DEV)
                fp = torch.empty(b, dtype=torch.int64, device=DEV)
                fn = torch.empty(b, dtype=torch.int64, device=DEV)
                g = torch.full((n, d), float("nan"), dtype=torch.float32, device=DEV)
                ws_bytes = lib.gnf_adj_loss_workspace_bytes(b, n, cap)
                ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
                _abi.check(lib.gnf_adj_loss_f32(C.byref(desc), _abi.ptr(z), z.stride(0), d, cap, C.byref(spec), _abi.ptr(loss),
                                                _abi.ptr(sums2), _abi.ptr(fp), _abi.ptr(fn), _abi.ptr(g), d, 1.0, _abi.ptr(ws),
                                                ws_bytes, st), "gnf_adj_loss_f32")
                assert bool((ws[ws_bytes:] == 0xA5).all()), "gnf_adj_loss_f32 wrote past gnf_adj_loss_workspace_bytes"
                out[f"adj_loss/D{d}/{name}/{'soft' if soft else 'hard'}"] = _sha(loss, sums2, fp, fn, g)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    commit = os.environ.get("GNF_DIGESTS_COMMIT")    # (set it when GNF_LIB_PATH points at another checkout's build)
    if not commit:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    digests = measure()
    with open(OUT, "w") as f:
        json.dump({"commit": commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests from commit {commit} -> {OUT} ({os.path.getsize(OUT)} B)")
