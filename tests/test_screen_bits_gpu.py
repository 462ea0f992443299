"""The soft silhouette, its image terms, the z-buffer, the depth-order term and their callers in the fit compute, output for output
and bit for bit, what the library of commit bc24efb computed, before csrc/silhouette.hip and csrc/depth_order.hip were folded onto
csrc/screen_common.h: tests/golden/screen_bits.json (recorded by tests/golden/make_golden_screen_bits.py, which says why the file must
not be regenerated from this tree) against the cases of tests/_screen_bits.py."""
import json
import os

import pytest
import torch

import _screen_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "screen_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert list(golden["cases"]) == list(_screen_bits.CASES) and golden["commit"].startswith("bc24efb")


@pytest.mark.parametrize("name", list(_screen_bits.CASES))
def test_bits(hip_lib, cuda, golden, name):
    want = golden["cases"][name]
    got = _screen_bits.record(name, cuda)
    assert len(got) == len(want)
    differ = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, f"{name}: outputs {differ} of {len(want)} differ, the first: {got[differ[0]]} != {want[differ[0]]}"


def test_a_pose_alone_equals_its_row_of_the_batch(hip_lib, cuda):
    with torch.enable_grad():
        alpha3, grad3, alpha1, grad1 = _screen_bits.CASES["silhouette_batch"](cuda)
    assert alpha3.shape[0] == 3 and alpha1.dim() == 2
    assert torch.equal(alpha1, alpha3[0]) and torch.equal(grad1, grad3[0])
    assert not bool(alpha3[1].any()) and not bool(grad3[1].any())  # the pose off-screen
