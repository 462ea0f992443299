"""The deterministic half of the lift family - plan build, plan gather, fused low-res gather, mask band census - computes, output for
output and bit for bit, what it computed at commit 0c4d1fe, before the host side of lift.hip and the lift wrappers of ops.py were
folded onto shared helpers: tests/golden/lift_bits.json (recorded by tests/golden/make_golden_lift_bits.py, which says why the file
must not be regenerated from this tree) against the cases of tests/_lift_bits.py."""
import json
import os

import pytest

import _lift_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "lift_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert list(golden["cases"]) == list(_lift_bits.CASES) and golden["commit"].startswith("0c4d1fe")


@pytest.mark.parametrize("name", list(_lift_bits.CASES))
def test_bits(hip_lib, cuda, golden, name):
    want = golden["cases"][name]
    got = _lift_bits.record(name, cuda)
    assert len(got) == len(want)
    differ = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, f"{name}: outputs {differ} of {len(want)} differ, the first: {got[differ[0]]} != {want[differ[0]]}"
