"""The fused norms+SGD pass against a recording of its own bits.

tests/golden/group_pass_bits.json holds, per case of tools/record_group_pass_bits.py - every entry
point x update form, the scalar-path and missing-gradient variants of the momentum forms, the
clipped entry under a bound that clips, one that does not and a gradient with an inf with and
without the skip - three SHA-256 digests, one after each pass, over the raw bytes of the
parameters, the momentum buffers, the returned fp64 sums and the gate, rate and clip states.  It was
recorded on an MI355X from the kernels as they stood before the pass's twelve wrapper kernel
families became one template; the kernels here must reproduce every digest.  Criterion: equality."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_group_pass_bits",
                                               os.path.join(ROOT, "tools", "record_group_pass_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
CASES = rec.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "group_pass_bits.json")) as f:
        return json.load(f)


def test_recording_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)
    assert all(len(v) == rec.PASSES for v in golden.values())


@pytest.mark.parametrize("cid", list(CASES))
def test_pass_reproduces_recorded_bits(dev, golden, cid):
    got = rec.run_case(dev, CASES[cid])
    assert got == golden[cid], [k for k, (a, b) in enumerate(zip(got, golden[cid])) if a != b]
