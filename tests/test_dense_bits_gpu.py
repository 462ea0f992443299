"""The dense, data-movement and decode-attention wrappers of interactvlm_amd/ops.py compute, output for output and bit for bit, what
they computed at commit 37130e4, before they were folded onto one launch frame, one epilogue filler and one kind table:
tests/golden/dense_bits.json (recorded by tests/golden/make_golden_dense_bits.py, which says why the file must not be regenerated
from this tree) against the cases of tests/_dense_bits.py."""
import json
import os

import pytest

import _dense_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "dense_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert list(golden["cases"]) == list(_dense_bits.CASES) and golden["commit"].startswith("37130e4")


@pytest.mark.parametrize("name", list(_dense_bits.CASES))
def test_bits(hip_lib, cuda, golden, name):
    want = golden["cases"][name]
    got = _dense_bits.record(name, cuda)
    assert len(got) == len(want)
    differ = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, f"{name}: outputs {differ} of {len(want)} differ, the first: {got[differ[0]]} != {want[differ[0]]}"
