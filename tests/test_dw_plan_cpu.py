"""The weight-gradient (dW) launch plans of the backward walk, as gnf_dw_plan_describe reports them (include/gnf_dw_plan.h),
against the plans recorded from the library of the commit named in tests/golden/dw_plans.json - the planner as ONE function,
before it was taken apart into csrc/gnf_dw_plan.h.  Equality is exact: every figure of a plan is an index into caller memory
or decides the summation order of a gradient, so a refactor of the planner must not move one.

The entry point runs without a device (the CU count the policies consult falls back to 256 without one, which is also the
MI355X's).  Grid (tests/golden/make_dw_plans.py): the suite's 8 -> 32 x 3 nets, the bench's 64 / 256 x 5, the wide 200 / 2048 x 3
and 14 / 1280 x 3, edge attention with 8 heads of 10 and with one head of 64 / 64, graph-scope attention with Wo; n in {0, 1, 31,
32, 33, 255, 256, 257, 2718, 3072, 3073, 16385, 78 000} (+ 300 000 on the wide net: the one plan off the buffer path, and
6 000 on the bench's nets: the one the streams policy's budget sends back to the grouped kernel); the
streams, generic and merged routes (merged: with and without the tile workgroups, first and last half-step), dw_grouped,
dw_wide_units in {8, 13, 40, 64, 200, 640}, dw_thin_on_dw; accumulate 0 / 1.

Besides equality: invariants every plan must satisfy, worked out from the record alone - what the kernels assume of a plan
(dw_wide_body, k_gemm_dw_grouped, reduce_jobs_strided) without being able to check it."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_dw_plans", os.path.join(GOLDEN, "make_dw_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

WGM = WGN = 128   # the wide kernel's tile
WGK = 32          # its k-step (= the grouped kernel's)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "dw_plans.json")) as f:
        blob = json.load(f)
    assert len(blob["commit"]) == 40 and blob["plans"] == len(list(gen.cases()))
    return blob["groups"]


@pytest.fixture(scope="module")
def measured():
    return gen.measure()


def test_grid_is_the_recorded_one(recorded, measured):
    assert sorted(recorded) == sorted(gen.condensed(measured))
    assert gen.NODES == [0, 1, 31, 32, 33, 255, 256, 257, 2718, 3072, 3073, 16385, 78000]
    assert gen.WIDE_UNITS == [8, 13, 40, 64, 200, 640] and len(gen.NETS) == 7
    assert len(measured) == len(list(gen.cases())) > 2000
    assert sum(len(g["tags"].split()) for g in recorded.values()) == len(measured)


@pytest.mark.parametrize("net", sorted(gen.NETS))
def test_plans_equal_the_recorded_ones(net, recorded, measured):
    """exact: one sha256 per policy over every record of the net; the per-plan tags only say which plan moved"""
    bad = []
    for name, got in sorted(gen.condensed(measured).items()):
        want = recorded[name]
        if name.split("/")[0] != net or want["sha256"] == got["sha256"]:
            continue
        keys = [k for k in measured if k.split("/")[0::2] == name.split("/")]   # (the order the tags were written in)
        moved = [k for k, w, g in zip(keys, want["tags"].split(), got["tags"].split()) if w != g]
        now = gen.parse(measured[moved[0]]) if moved else None
        bad.append(f"{name}: {len(moved)} plans differ from the recorded ones: {moved[:12]}; the first one now: {now}")
    assert not bad, "\n".join(bad[:10])


def tiles_of(j):
    return -(-j["M"] // WGM) * -(-j["N"] // WGN)


def check_plan(key, p):
    """the invariants of one parsed plan; -> list of violations"""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(f"{key}: {what}")

    n, nj, wide = p["n"], p["nj"], p["wide"]
    lo = p["wslab"] + p["slab_set"] * p["slab_stride"]
    need(p["slab_set"] < p["slab_sets"], "slab set out of range")
    need(sorted(j["job"] for j in p["jobs"]) == list(range(nj)), "the launch order is not a permutation of the job list")
    # ---- slabs: room and place ---------------------------------------------------------------------------------------
    regions = []
    for q, j in enumerate(p["jobs"]):
        need(1 <= j["chunks"] <= p["slab_chunks"], f"job {q}: {j['chunks']} chunks, room for {p['slab_chunks']}")
        for ptr, size in ((j["C"], j["M"] * j["N"]), (j["aux"], j["N"])):
            if ptr >= 0:
                regions.append((ptr, ptr + j["chunks"] * size, q))
                need(lo <= ptr and ptr + j["chunks"] * size <= lo + p["slab_stride"], f"job {q}: slab outside its set")
        red = p["reduce"][j["job"]]
        need((j["C"] == red["gw"]) == (j["C"] < 0), f"job {q}: C is neither a slab nor its own gradient")
        need(j["aux"] in (-1, red["gb"]) or j["aux"] >= 0, f"job {q}: the column sums go to another job's bias gradient")
        need((j["aux"] == -1) == (red["gb"] == -1), f"job {q}: column sums without a bias gradient (or the reverse)")
        if j["C"] >= 0:   # left for the reduce: it must read what the GEMM writes
            need((red["wslab"], red["nw"], red["chunks"]) == (j["C"], j["M"] * j["N"], j["chunks"]), f"job {q}: the reduce reads another slab")
            need(red["bslab"] == j["aux"] and red["nb"] == (j["N"] if j["aux"] >= 0 else 0), f"job {q}: the reduce reads another bias slab")
        elif wide:        # written in place by the wide kernel: nothing left to add
            need(red["nw"] == 0 and red["nb"] == 0 and j["chunks"] == 1 and not p["accumulate"], f"job {q}: in place, but reduced / cut / accumulating")
    regions.sort()
    for a, b in zip(regions, regions[1:]):
        need(a[1] <= b[0], f"slabs of jobs {a[2]} and {b[2]} overlap")
    # ---- direct: only if no job is left for the reduce ------------------------------------------------------------------
    if p["direct"]:
        need(all(j["C"] < 0 for j in p["jobs"]) and not p["accumulate"], "direct, but a job writes a slab (or accumulates)")
    if wide:
        need(p["direct"] == all(r["nw"] == 0 and r["nb"] == 0 for r in p["reduce"]), "direct != nothing left for the reduce")
    # ---- the cut ----------------------------------------------------------------------------------------------------------
    sk_jobs = p["sk_jobs"] if wide else 0
    for q, j in enumerate(p["jobs"]):
        if q < sk_jobs:
            continue
        c, kc = j["chunks"], j["kchunk"]
        need(kc % WGK == 0 and kc >= WGK, f"job {q}: kchunk {kc} is no multiple of {WGK}")
        need(c * kc >= n > (c - 1) * kc if n > 0 else c == 1, f"job {q}: {c} chunks of {kc} rows do not cut {n} rows")
    if wide:
        need(n > 0 and p["units"] >= 1, "a wide plan of nothing")
        base = 0
        for q, j in enumerate(p["jobs"]):
            need(j["gx"] == -(-j["N"] // WGN), f"job {q}: gx")
            need(j["unit_base"] == base, f"job {q}: unit_base {j['unit_base']}, {base} units in front of it")
            base += tiles_of(j) * (1 if q < sk_jobs else j["chunks"])
        need(p["unit_end"] == base, f"unit_base ends at {p['unit_end']}, the jobs have {base} units")
        need(p["units"] <= max(base, 1) or p["sk_q"] > 0, "more workgroups than units")
        need(p["xcd_jobs"] == 0 or (p["units"] % 8 == 0 and p["sk_q"] == 0), "XCD blocks without a multiple of 8 workgroups")
        for q in range(p["xcd_jobs"]):
            j = p["jobs"][q]
            need(j["chunks"] == 1 and tiles_of(j) % 8 == 0 and j["unit_base"] % 8 == 0, f"job {q}: not an XCD-block job")
    else:
        need(p["nz"] == nj * p["plan_chunks"] and all(j["chunks"] == p["plan_chunks"] for j in p["jobs"]), "grouped: chunks")
        need(p["groups"] * p["rpg"] >= p["gy"] and p["blocks"] >= p["nz"] * p["groups"] * p["gx"] * p["rpg"], "grouped: the grid does not cover the bands")
        need(p["gx"] == max([-(-j["N"] // 64) for j in p["jobs"]] + [1]) and p["gy"] == max([-(-j["M"] // 128) for j in p["jobs"]] + [1]), "grouped: tile grid")
    # ---- stream-K -----------------------------------------------------------------------------------------------------------
    if wide and p["sk_q"] > 0:
        q_, steps, tiles = p["sk_q"], p["sk_steps"], p["sk_tiles"]
        need(steps == -(-n // WGK) and q_ <= steps, f"sk_q {q_} > sk_steps {steps}")
        need(tiles == sum(tiles_of(j) for j in p["jobs"][:sk_jobs]) and p["sk_light_base"] == tiles, "sk_tiles / sk_light_base")
        total = tiles * steps
        # workgroup b runs steps [b sk_q, min((b + 1) sk_q, total)): every step once, no workgroup of `units` left without
        need((p["units"] - 1) * q_ < total <= p["units"] * q_, f"{p['units']} runs of {q_} steps do not cover {total} steps exactly once")
        t = 0
        for q, j in enumerate(p["jobs"][:sk_jobs]):
            need(j["kchunk"] == q_ * WGK, f"job {q}: stream-K kchunk")
            for _ in range(tiles_of(j)):
                pieces = ((t + 1) * steps - 1) // q_ - (t * steps) // q_ + 1
                need(pieces <= j["chunks"], f"job {q}: tile {t} is touched by {pieces} pieces, {j['chunks']} slabs")
                t += 1
        need(not p["light_on_tiles"] or sk_jobs < nj, "light_on_tiles without thin jobs")
    else:
        need(not (p["sk_q"] or p["sk_jobs"] or p["light_on_tiles"] or p["sk_tiles"]), "stream-K fields of a whole-chunk plan")
    # ---- the reduce's index space ----------------------------------------------------------------------------------------------
    quads = 0
    for e, r in enumerate(p["reduce"]):
        need(p["qpre"][e] == quads, f"qpre[{e}] = {p['qpre'][e]}, {quads} items in front of it")
        if r["nw"] % 4 == 0 and r["wslab"] % 4 == 0:   # (the synthetic gradient buffers are 16-byte aligned)
            quads += r["nw"] // 4
    need(p["qpre"][nj] == quads == p["items"], "qpre's end")
    need(4 * p["items"] + p["singles"] == sum(r["nw"] + r["nb"] for r in p["reduce"]), "qpre and singles do not add up to the reduce items")
    need(p["maxred"] == max([j["M"] * j["N"] + (j["N"] if p["reduce"][j["job"]]["gb"] != -1 else 0) for j in p["jobs"]] + [1]), "maxred")
    return bad


def test_invariants_hold_on_every_plan(measured):
    bad = []
    for key in sorted(measured):
        bad += check_plan(key, gen.parse(measured[key]))
    assert not bad, f"{len(bad)} violations\n" + "\n".join(bad[:30])


def test_grid_reaches_every_branch(recorded):
    """the recorded plans are not all of one kind: every branch of the planner (make_dw_plans.KINDS: wide whole-chunk,
    stream-K, thin jobs on the tile workgroups, XCD blocks, direct, off the buffer path, grouped by budget and by option,
    an accumulating wide plan, slab room beyond the plan's chunks) is taken by at least one of them"""
    for kind in gen.KINDS:
        assert sum(g["kinds"].get(kind, 0) for g in recorded.values()) > 0, kind


def test_entry_point_is_declared_bound_and_refuses_bad_arguments():
    import ctypes as C
    import re
    from gnf_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "gnf.h")).read()
    assert re.search(r'^#include "gnf_dw_plan.h"$', main, flags=re.M) and re.search(r"^#define GNF_ABI_VERSION 10$", main, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gnf_dw_plan.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(gnf_[a-z0-9_]+)\s*\(", text))) == ["gnf_dw_plan_describe"] == list(_abi.DW_PLAN_SYMBOLS)
    assert len(_abi.EXPORTED_SYMBOLS) == 41 and _abi.lib().gnf_abi_version() == 10
    mlp, keep = gen._mlp(_abi, "mp_8_32x3")
    f, buf = _abi.lib().gnf_dw_plan_describe, (C.c_int64 * 1024)()
    assert f(40, 8, C.byref(mlp), gen.STREAMS, 0, 0, 0, 0, 0, 0, buf, 1024) == len(gen.HEADER) + 6 * 20 + 7 and buf[0] == 1
    assert f(40, 8, C.byref(mlp), gen.STREAMS, 0, 0, 0, 0, 0, 0, buf, 10) == -1      # cap too small
    assert "cap 10" in _abi.lib().gnf_last_error().decode()
    assert f(40, 7, C.byref(mlp), gen.STREAMS, 0, 0, 0, 0, 0, 0, buf, 1024) == -1    # odd D
    assert f(40, 8, None, gen.STREAMS, 0, 0, 0, 0, 0, 0, buf, 1024) == -1
    assert f(40, 8, C.byref(mlp), 3, 0, 0, 0, 0, 0, 0, buf, 1024) == -1              # no such route
    assert f(40, 8, C.byref(mlp), gen.MERGED, 3, gen.TILE_LDS, 0, 0, 2, 0, buf, 1024) == -1   # two slab sets
    assert f(4000, 8, C.byref(mlp), gen.STREAMS, 0, 0, 0, 0, 1, 0, buf, 1024) == -1  # one slab set above 192 tiles
