"""The totals of the three caller-memory layouts (csrc/gnf_layout.h: half-step scratch, attention region / stash slot,
MLP-row stash slot) and of the backward plan, as the size entry points report them, against values recorded from the
library of the commit named in tests/golden/workspace_sizes.json.  Equality is exact: a refactor of the layout code must
not move a byte.

All six entry points run without a device (the CU count they consult falls back to 256 without one, which is also the
MI355X's), so none is left to the GPU suite.  Grid (tests/golden/make_workspace_sizes.py): n in {0, 1, 15, 16, 17, 2718,
78 000}; message-passing nets with eps and concat combine, the bench's latent 256 x K 5 and the wide 2048 x 3 net (layered
path, layered stash mode); edge-scope attention with the drivers' 8 heads and the data driver's one head of 64 / 64;
graph-scope attention with and without Wo; T in {1, 8}; weight sharing on / off; with and without bns."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_workspace_sizes", os.path.join(GOLDEN, "make_workspace_sizes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "workspace_sizes.json")) as f:
        blob = json.load(f)
    assert len(blob["commit"]) == 40 and blob["functions"] == gen.FUNCS
    return blob["sizes"]


@pytest.fixture(scope="module")
def measured():
    return gen.measure()


def test_grid_is_the_recorded_one(recorded, measured):
    assert sorted(recorded) == sorted(measured)
    assert len(measured) == len(gen.NETS) * len(gen.TIMESTEPS) * 2 * 2 * len(gen.NODES)
    assert gen.NODES == [0, 1, 15, 16, 17, 2718, 78000] and gen.TIMESTEPS == [1, 8]


@pytest.mark.parametrize("net", sorted(gen.NETS))
def test_sizes_equal_the_recorded_ones(net, recorded, measured):
    bad = []
    for key in sorted(measured):
        if key.split("/")[0] != net:
            continue
        for fn, want, got in zip(gen.FUNCS, recorded[key], measured[key]):
            if want != got:
                bad.append(f"{fn} {key}: {got} != recorded {want}")
    assert not bad, "\n".join(bad[:20])


def test_grid_reaches_every_layout(recorded):
    """the recorded values are not trivially zero where a layout applies: both stash modes, the attention stash of the
    edge scope only, and every workspace"""
    def at(net, n, t=8, share=0, bn=0):
        return dict(zip(gen.FUNCS, recorded[gen.key_of(net, t, share, bn, n)]))
    assert at("mp_bench_256x5", 2718)["gnf_mlp_stash_bytes"] > 0          # fused mode (one 16-node tile per CU at most)
    assert at("mp_bench_256x5", 78000)["gnf_mlp_stash_bytes"] == 0
    assert at("mp_wide_2048x3", 2718)["gnf_mlp_stash_bytes"] > 0          # layered mode
    assert at("attn_edges_8x10", 2718)["gnf_attn_stash_bytes"] > 0
    assert at("attn_edges_1x64_data_driver", 2718)["gnf_attn_stash_bytes"] > 0
    assert at("attn_graph_wo", 2718)["gnf_attn_stash_bytes"] == 0         # the graph scope declines the stash
    for net in gen.NETS:
        for fn in ("gnf_workspace_bytes", "gnf_gnn_workspace_bytes", "gnf_per_graph_workspace_bytes", "gnf_backward_workspace_bytes"):
            assert at(net, 17)[fn] > 0, (net, fn)
