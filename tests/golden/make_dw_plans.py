#!/usr/bin/env python3
"""Record the weight-gradient (dW) launch plans of the backward walk, as gnf_dw_plan_describe reports them, over the grid of
tests/test_dw_plan_cpu.py.

    python tests/golden/make_dw_plans.py            # -> tests/golden/dw_plans.json

The plans are host computations (no device is touched; without one the CU count the policies consult falls back to 256, the
MI355X's own), so the file pins every figure that reaches a dW kernel or launch: a change of the planner that moves one of
them fails tests/test_dw_plan_cpu.py until the file is regenerated ON PURPOSE, from a build of the commit named in it.
The file in the repository was recorded from the commit that added gnf_dw_plan_describe to the planner as it then stood
(the parent of the planner's refactoring into csrc/gnf_dw_plan.h plus the entry point, nothing else), so it describes the
one-function planner's behaviour and not the code under test.
GNF_LIB_PATH selects a library built from another checkout (gnf_amd/_abi.py); name its commit in GNF_PLANS_COMMIT.

The file keeps digests, not plans (written out, the grid's records are 4 MB): per net and policy one sha256 over the
records of all its node counts and accumulate flags, a 32-bit tag per plan to tell which one moved, and the number of
plans that took each branch of the planner (KINDS).
"""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dw_plans.json")

FAKE = 0x1000                     # the planner reads shapes and whether a pointer is NULL, never through one
HEADER = ("version n nj wide buf direct units lds maxred "
          "plan_chunks plan_kchunk slab_chunks slab_sets slab_set wslab bslab slab_stride wsum osum "
          "sk_q sk_steps sk_tiles sk_jobs sk_light_base xcd_jobs light_on_tiles unit_end "
          "accumulate singles items gx gy nz groups rpg blocks").split()
JOB = "job M N gx chunks kchunk unit_base lda ldb A B C aux".split()
RED = "nw nb chunks wslab bslab gw gb".split()
STREAMS, MERGED, GENERIC = 0, 1, 2

# name -> D, MLP widths, attention block (heads, kq, v, out, concat, kq_division, scope, Wo)
NETS = {
    "mp_8_32x3": dict(D=8, dims=[4, 32, 32, 4]),                                  # the suite's MP
    "mp_64_256x5": dict(D=64, dims=[32, 256, 256, 256, 256, 32]),                 # the bench's config 2
    "mp_200_2048x3": dict(D=200, dims=[100, 2048, 2048, 100]),                    # wide_fc
    "mp_14_1280x3": dict(D=14, dims=[7, 1280, 1280, 7]),
    "attn_edges_8x10": dict(D=64, dims=[112, 256, 256, 256, 256, 32], attn=(8, 10, 10, 80, 1, 0, 0, True)),
    "attn_edges_1x64": dict(D=200, dims=[164, 2048, 2048, 100], attn=(1, 64, 64, 64, 1, 1, 0, True)),
    "attn_graph_wo": dict(D=64, dims=[112, 256, 256, 256, 256, 32], attn=(8, 10, 10, 80, 1, 1, 1, True)),
}
NODES = [0, 1, 31, 32, 33, 255, 256, 257, 2718, 3072, 3073, 16385, 78000]
# The operands' leading dimensions are the plan's own (layer widths), so the buffer path's 2^31-byte bound is reached by the
# batch, not by a padded stride: one case beyond the grid, the wide net's whole-node-axis chunks at 300 000 nodes.
# And one batch of the bench's nets that the fused backward walks in 32-node tiles (more than 256 tiles of 16): 188 exclusive
# workgroups leave the wide kernel 64, whose cut the streams policy estimates slower than its budget - the grouped kernel.
EXTRA_NODES = {"mp_200_2048x3": [300000], "mp_64_256x5": [6000]}
WIDE_UNITS = [8, 13, 40, 64, 200, 640]
TILE_LDS = 100 * 1024             # LDS of a backward tile workgroup: above the 80 KB that make it exclusive on its CU

# name -> route, library options, stashed, last, slab_set.  "tiles": the route is planned around the fused backward launch
# (16-node tiles) where the net has one - message-passing nets with hidden layers below 512 - as the walk does
POLICIES = {
    "streams": dict(route=STREAMS),
    "generic": dict(route=GENERIC),
    "grouped": dict(route=STREAMS, opts=dict(dw_grouped=1)),
    **{f"streams_units{u}": dict(route=STREAMS, opts=dict(dw_wide_units=u)) for u in WIDE_UNITS},
    "merged_stash": dict(route=MERGED, stashed=1, slab_set=1),
    "merged_stash_last": dict(route=MERGED, stashed=1, last=1),
    "merged_stash_thin_on_dw": dict(route=MERGED, stashed=1, slab_set=1, opts=dict(dw_thin_on_dw=1)),
    "merged_recompute": dict(route=MERGED, slab_set=1),
    "merged_recompute_last": dict(route=MERGED, last=1),
    **{f"merged_stash_units{u}": dict(route=MERGED, stashed=1, opts=dict(dw_wide_units=u)) for u in (8, 13, 200)},
}


def hidden_max(dims):
    return max(dims[1:-1])


def cases():
    """(key, net, n, policy name, accumulate): the merged route where the walk can take it - nets the fused kernels hold, up
    to 192 tiles, a non-empty batch"""
    for net, c in NETS.items():
        for n in NODES + EXTRA_NODES.get(net, []):
            for pol, spec in POLICIES.items():
                if spec["route"] == MERGED and (hidden_max(c["dims"]) >= 512 or not 0 < n <= 3072):
                    continue
                if n == 300000 and pol != "generic":
                    continue
                for acc in (0, 1):
                    yield f"{net}/n{n}/{pol}/acc{acc}", net, n, pol, acc


def launch_around(net, n, pol):
    """(workgroups, LDS bytes) of the backward launch the policy is shaped around, (0, 0) where there is none"""
    c, route = NETS[net], POLICIES[pol]["route"]
    fused = "attn" not in c and hidden_max(c["dims"]) < 512
    tiles = (n + 15) // 16 if (n + 15) // 16 <= 256 else (n + 31) // 32    # (one or two 16-node tiles per workgroup)
    return (tiles, TILE_LDS) if route == MERGED or (route == STREAMS and fused) else (0, 0)


def _mlp(_abi, name):
    """-> (GnfMlp, what must stay alive while it is used)"""
    c = NETS[name]
    m = _abi.GnfMlp()
    m.num_layers = len(c["dims"]) - 1
    for j, d in enumerate(c["dims"]):
        m.dims[j] = d
    for j in range(m.num_layers):
        m.W[j] = m.b[j] = FAKE
    m.packed = FAKE
    at = None
    if "attn" in c:
        at = _abi.GnfAttn()
        (at.num_heads, at.kq_dim, at.v_dim, at.out_dim, at.concat, at.kq_dim_division, at.scope, wo) = c["attn"]
        at.Wq = at.Wk = at.Wv = FAKE
        at.Wo = FAKE if wo else None
        m.attn = C.pointer(at)
    return m, at


def describe(_abi, mlp, d, n, route, tiles=0, lds=0, stashed=0, last=0, slab_set=0, acc=0):
    """one call of gnf_dw_plan_describe -> the record as a list of ints"""
    buf = (C.c_int64 * 1024)()
    got = _abi.lib().gnf_dw_plan_describe(n, d, C.byref(mlp), route, tiles, lds, stashed, last, slab_set, acc, buf, len(buf))
    _abi.check(min(got, 0), "gnf_dw_plan_describe")
    return list(buf[:got])


def measure():
    """{key: record} from the library gnf_amd._abi loads; every option a policy sets is reset afterwards"""
    from gnf_amd import _abi
    out = {}
    for key, net, n, pol, acc in cases():
        c, spec = NETS[net], POLICIES[pol]
        mlp, keep = _mlp(_abi, net)
        tiles, lds = launch_around(net, n, pol)
        opts = spec.get("opts", {})
        try:
            for k, v in opts.items():
                _abi.set_option(k, v)
            out[key] = describe(_abi, mlp, c["D"], n, spec["route"], tiles, lds,
                                spec.get("stashed", 0), spec.get("last", 0), spec.get("slab_set", 0), acc)
        finally:
            for k in opts:
                _abi.set_option(k, 0)
        del keep
    return out


def parse(rec):
    """a record -> dict of the header's fields + "jobs" (launch order) / "reduce" (job-list order): dicts, + "qpre" """
    h = dict(zip(HEADER, rec))
    nj, at = h["nj"], len(HEADER)
    h["jobs"] = [dict(zip(JOB, rec[at + len(JOB) * q:])) for q in range(nj)]
    at += len(JOB) * nj
    h["reduce"] = [dict(zip(RED, rec[at + len(RED) * e:])) for e in range(nj)]
    at += len(RED) * nj
    h["qpre"] = rec[at:at + nj + 1]
    assert at + nj + 1 == len(rec), (at, nj, len(rec))
    return h


def digest(rec):
    return hashlib.sha256(struct.pack(f"<{len(rec)}q", *rec)).hexdigest()


KINDS = ("wide_whole_chunks", "stream_k", "light_on_tiles", "xcd_blocks", "wide_direct", "grouped_direct", "wide_no_buf",
         "grouped_by_budget", "grouped_by_option", "wide_accumulate", "extra_slab_room")


def kinds(key, rec):
    """which of the planner's branches a plan took (the names of KINDS)"""
    h, (net, _, pol, _) = dict(zip(HEADER, rec)), key.split("/")
    wide = h["wide"]
    return [k for k, hit in zip(KINDS, (
        wide and not h["sk_q"], wide and h["sk_q"] > 0, h["light_on_tiles"], h["xcd_jobs"] > 0, wide and h["direct"],
        not wide and h["direct"], wide and not h["buf"],
        # the streams policy offered the wide kernel (1 .. 192 exclusive workgroups around it, no option set) and the cut it
        # allowed was estimated slower than its budget
        not wide and pol == "streams" and 0 < launch_around(net, h["n"], pol)[0] <= 192,
        not wide and pol == "grouped", wide and h["accumulate"], h["slab_chunks"] > h["plan_chunks"])) if hit]


def condensed(plans):
    """what the file keeps of {key: record}: per net and policy ONE sha256 over the records of its node counts and accumulate
    flags (exact equality), a 32-bit tag per plan in that order (which of them moved), and how many took each branch (KINDS)"""
    out = {}
    for key in plans:   # (cases() order: node counts ascending, accumulate 0 / 1)
        net, n, pol, acc = key.split("/")
        g = out.setdefault(f"{net}/{pol}", {"sha256": hashlib.sha256(), "tags": [], "kinds": {}})
        g["sha256"].update(digest(plans[key]).encode())
        g["tags"].append(digest(plans[key])[:8])
        for k in kinds(key, plans[key]):
            g["kinds"][k] = g["kinds"].get(k, 0) + 1
    return {name: {"sha256": g["sha256"].hexdigest(), "tags": " ".join(g["tags"]), "kinds": g["kinds"]} for name, g in out.items()}


if __name__ == "__main__":
    commit = os.environ.get("GNF_PLANS_COMMIT")      # (set it when GNF_LIB_PATH points at another checkout's build)
    if not commit:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    plans = measure()
    groups = condensed(plans)

    def dumps(v):
        return json.dumps(v, separators=(",", ":"), sort_keys=True)
    with open(OUT, "w") as f:   # one net and policy per line
        f.write('{"commit":%s,\n"plans":%d,\n"groups":{\n' % (dumps(commit), len(plans)))
        f.write(",\n".join(f"{dumps(k)}:{dumps(groups[k])}" for k in sorted(groups)))
        f.write("\n}}\n")
    print(f"{len(plans)} plans in {len(groups)} groups from commit {commit} -> {OUT} ({os.path.getsize(OUT)} B)")
