"""The decoders and the adjacency loss reproduce, bit for bit, what the commit named in tests/golden/pair_family_digests.json
computed on the MI355X: raw ctypes calls to gnf_pred_adj_f32, gnf_adj_edges_count_f32 + gnf_adj_edges_fill (thresholds 0.1 /
0.5 / 0.9) and gnf_adj_loss_f32 with a gradient, on the 198 nodes of adj_loss_ref.SIZES at D = 7, 200, 400, 1030 - one per
instance of the pair kernel, both routes of the decode kernels - the loss over (10, 1, scaled), (10, 1, unscaled) and
(3, 2, scaled) with hard and soft labels (tests/golden/make_pair_family_digests.py makes the calls; here they are made
again and the sha256 of every output's bytes is compared).  gnf_adj_loss_f32 is also held to its own workspace size: a guard
band behind it stays untouched.

The digests pin the toolchain's expf and log1pf as much as the kernels: a ROCm upgrade that changes either re-records the file,
on purpose, from a build of the commit it names (the script's docstring says how)."""
import importlib.util
import json
import os

import pytest
import torch

from gnf_amd import _abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pair_family_digests", os.path.join(GOLDEN, "make_pair_family_digests.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


def test_every_output_has_the_recorded_bits():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _abi.lib()
    with open(os.path.join(GOLDEN, "pair_family_digests.json")) as f:
        golden = json.load(f)
    want = golden["digests"]
    assert len(want) == len(maker.DIMS) * (1 + len(maker.THRESHOLDS) + 2 * len(maker.SPECS)) == 40
    got = maker.measure()
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    print(f"[pair family] {len(want) - len(wrong)} of {len(want)} digests equal those of commit {golden['commit'][:12]}")
    assert not wrong, wrong
