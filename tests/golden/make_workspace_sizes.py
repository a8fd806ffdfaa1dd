#!/usr/bin/env python3
"""Record what the library's size entry points return, over the grid of tests/test_layout_cpu.py.

    python tests/golden/make_workspace_sizes.py            # -> tests/golden/workspace_sizes.json

The sizes are host computations (no device is touched; without one the CU count they consult falls back to 256, the
MI355X's own), so the file pins every workspace / stash layout's total: a change of the library that moves one of them
fails tests/test_layout_cpu.py until the file is regenerated ON PURPOSE, from a build of the commit named in it.
GNF_LIB_PATH selects a library built from another checkout (gnf_amd/_abi.py); name its commit in GNF_SIZES_COMMIT.
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_sizes.json")

NODES = [0, 1, 15, 16, 17, 2718, 78000]
N_GRAPHS = 64                     # gnf_per_graph_workspace_bytes (0 graphs for the empty batch)
FAKE = 0x1000                     # the size functions read shapes and whether a pointer is NULL, never through one

# name -> D, MLP widths, combine, packed copies present, attention block (heads, kq, v, out, concat, kq_division, scope, Wo)
NETS = {
    "mp_eps_small": dict(D=8, dims=[4, 32, 4], combine=0, packed=False),
    "mp_concat_small": dict(D=8, dims=[8, 32, 32, 4], combine=1, packed=True),
    "mp_bench_256x5": dict(D=64, dims=[32, 256, 256, 256, 256, 32], combine=0, packed=True),
    "mp_bench_256x5_concat": dict(D=64, dims=[64, 256, 256, 256, 256, 32], combine=1, packed=True),
    "mp_wide_2048x3": dict(D=200, dims=[100, 2048, 2048, 100], combine=0, packed=True),
    "attn_edges_8x10": dict(D=64, dims=[112, 256, 256, 256, 256, 32], combine=0, packed=True,
                            attn=(8, 10, 10, 80, 1, 0, 0, True)),
    "attn_edges_8x10_d8": dict(D=8, dims=[84, 64, 64, 4], combine=0, packed=True, attn=(8, 10, 10, 80, 1, 0, 0, True)),
    "attn_edges_1x64_data_driver": dict(D=200, dims=[164, 2048, 2048, 100], combine=0, packed=True,
                                        attn=(1, 64, 64, 64, 1, 1, 0, True)),
    "attn_graph_wo": dict(D=64, dims=[112, 256, 256, 256, 256, 32], combine=0, packed=True,
                          attn=(8, 10, 10, 80, 1, 1, 1, True)),
    "attn_graph_no_wo": dict(D=64, dims=[112, 256, 256, 256, 256, 32], combine=0, packed=True,
                             attn=(8, 10, 10, 80, 1, 1, 1, False)),
}
TIMESTEPS = [1, 8]
FUNCS = ["gnf_workspace_bytes", "gnf_gnn_workspace_bytes", "gnf_per_graph_workspace_bytes", "gnf_attn_stash_bytes",
         "gnf_mlp_stash_bytes", "gnf_backward_workspace_bytes"]


def case_keys():
    for name in NETS:
        for t in TIMESTEPS:
            for sharing in (0, 1):
                for bn in (0, 1):
                    yield name, t, sharing, bn


def key_of(name, t, sharing, bn, n):
    return f"{name}/T{t}/share{sharing}/bn{bn}/n{n}"


def _flow(_abi, name, t, sharing, bn):
    """-> (GnfFlow, everything that must stay alive while it is used)"""
    c = NETS[name]
    at = None
    if "attn" in c:
        at = _abi.GnfAttn()
        (at.num_heads, at.kq_dim, at.v_dim, at.out_dim, at.concat, at.kq_dim_division, at.scope, wo) = c["attn"]
        at.Wq = at.Wk = at.Wv = FAKE
        at.Wo = FAKE if wo else None
    count = 2 if sharing else 2 * t
    nets = (_abi.GnfMlp * count)()
    for m in nets:
        m.num_layers = len(c["dims"]) - 1
        for j, d in enumerate(c["dims"]):
            m.dims[j] = d
        for j in range(m.num_layers):
            m.W[j] = m.b[j] = FAKE
        m.packed = FAKE if c["packed"] else None
        if at is not None:
            m.attn = C.pointer(at)
    bns = (_abi.GnfBatchNorm * (2 * t))() if bn else None
    flow = _abi.GnfFlow(t, sharing, C.cast(nets, C.POINTER(_abi.GnfMlp)), C.cast(nets, C.POINTER(_abi.GnfMlp)),
                        _abi.GnfGnnSpec(1, c["combine"], 1.0, 1, 0.2))
    if bn:
        flow.bns = C.cast(bns, C.POINTER(_abi.GnfBatchNorm))
    return flow, (nets, at, bns)


def measure():
    """{key: [the six sizes, in FUNCS' order]} from the library gnf_amd._abi loads"""
    from gnf_amd import _abi
    lib = _abi.lib()
    out = {}
    for name, t, sharing, bn in case_keys():
        flow, keep = _flow(_abi, name, t, sharing, bn)
        d = NETS[name]["D"]
        for n in NODES:
            out[key_of(name, t, sharing, bn, n)] = [
                lib.gnf_workspace_bytes(n, d, C.byref(flow)),
                lib.gnf_gnn_workspace_bytes(n, d // 2, C.byref(keep[0][0]), NETS[name]["combine"]),
                lib.gnf_per_graph_workspace_bytes(n, N_GRAPHS if n else 0, d, C.byref(flow)),
                lib.gnf_attn_stash_bytes(n, d, C.byref(flow)),
                lib.gnf_mlp_stash_bytes(n, d, C.byref(flow)),
                lib.gnf_backward_workspace_bytes(n, d, C.byref(flow)),
            ]
    return out


if __name__ == "__main__":
    commit = os.environ.get("GNF_SIZES_COMMIT")      # (set it when GNF_LIB_PATH points at another checkout's build)
    if not commit:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    sizes = measure()
    with open(OUT, "w") as f:
        json.dump({"commit": commit, "functions": FUNCS, "sizes": sizes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(sizes)} cases x {len(FUNCS)} sizes from commit {commit} -> {OUT} ({os.path.getsize(OUT)} B)")
