"""The forward and inverse walk reproduces, bit for bit and on the same kernels, what the commit named in
tests/golden/walk_digests.json computed on the MI355X: GRevNet.f / g / f_per_graph / g_per_graph and one training step per
net family over the cases of tests/golden/make_walk_digests.py - fused and layered message passing, the compile-time-geometry
instance, weight sharing at T = 3, T = 1, a padded nodes view, batch norm as passes of its own and applied on load, the
packed and the two-launch attention front-ends, layer norm, graph-scope attention, the node-count thresholds of the
sum z^2 and moments ride-alongs, the large-batch kernel, the empty batch.  The calls are made again here; the sha256 of
every output's bytes and the route bits gnf_last_route reports are compared with the file.

The digests pin the toolchain's expf as much as the kernels: a ROCm upgrade that changes it re-records the file, on purpose,
from a build of the commit it names (the script's docstring says how)."""
import importlib.util
import json
import os

import pytest
import torch

from gnf_amd import _abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_walk_digests", os.path.join(GOLDEN, "make_walk_digests.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


def test_every_call_has_the_recorded_bits_and_route():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _abi.lib()
    with open(os.path.join(GOLDEN, "walk_digests.json")) as f:
        golden = json.load(f)
    want = golden["digests"]
    recorded = sorted({k.split("/")[0] for k in want})
    assert set(c[0] for c in maker.CASES) - set(recorded) <= set(maker.MAY_BE_UNSTABLE)
    got = maker.measure(only=recorded)
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    for k in wrong:
        print(f"[walk bits] {k}: got {got[k]}\n{' ' * 12}want {want[k]}")
    print(f"[walk bits] {len(want) - len(wrong)} of {len(want)} calls equal those of commit {golden['commit'][:12]}")
    assert not wrong, wrong
