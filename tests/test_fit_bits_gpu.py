"""The object-pose fit family computes, output for output and bit for bit, what it computed at commit 25cdd93, before its Python side
was rewritten around shared helpers: tests/golden/fit_bits.json (recorded by tests/golden/make_golden_fit_bits.py, which says why
the file must not be regenerated from this tree) against the cases of tests/_fit_bits.py."""
import json
import os

import pytest
import torch

import _fit_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "fit_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert list(golden["cases"]) == list(_fit_bits.CASES) and golden["commit"].startswith("25cdd93")


@pytest.mark.parametrize("name", list(_fit_bits.CASES))
def test_bits(hip_lib, cuda, golden, name):
    want = golden["cases"][name]
    with torch.enable_grad():
        got = _fit_bits.record(name, cuda)
    assert len(got) == len(want)
    differ = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, f"{name}: outputs {differ} of {len(want)} differ, the first: {got[differ[0]]} != {want[differ[0]]}"
