"""contact_distance without a GPU: the module imports, arguments are validated before the library is touched, and the C ABI
declares the entry points with the chain constant the Python side (and the GPU tests' tolerance) uses."""
import re

import pytest
import torch

from interactvlm_amd import _lib
from interactvlm_amd import contact_pair as cp


def test_module_imports_without_gpu():
    assert callable(cp.contact_distance) and callable(cp.contact_agreement)
    assert isinstance(cp.L_CHAIN, int) and 0 < cp.L_CHAIN <= 1024


def test_header_declares_the_entry_points():
    protos = _lib.header_prototypes()
    assert "ivlm_contact_pair" in protos and "ivlm_contact_pair_workspace_bytes" in protos
    ret, args = protos["ivlm_contact_pair"]
    assert ret == "int" and len(args) == 16
    assert protos["ivlm_contact_pair_workspace_bytes"][0] == "size_t"
    m = re.search(r"#define\s+IVLM_CONTACT_PAIR_CHAIN\s+(\d+)", open(_lib.HEADER_PATH).read())
    assert m and int(m.group(1)) == cp.L_CHAIN


def test_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.ivlm_contact_pair(None, None, None, None, 0, 1, 4, 4, 0, 0, None, None, None, None, 0, None) == -1
    assert lib.ivlm_contact_pair_workspace_bytes(1, 70, 33) > 0
    assert lib.ivlm_contact_pair_workspace_bytes(0, 70, 33) == 0
    # no [N_o, N_h] array: the workspace of the largest case of the issue stays far below one dense fp32 matrix
    assert lib.ivlm_contact_pair_workspace_bytes(1, 20000, 6890) < 20000 * 6890 * 4 // 50


def test_validation_raises_before_touching_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    o, h, p, q = torch.zeros(7, 3), torch.zeros(5, 3), torch.ones(7), torch.ones(5)
    with pytest.raises(_lib.IvlmError):  # CPU tensors: no CPU fallback
        cp.contact_distance(o, h, p, q)
    with pytest.raises(ValueError):
        cp.contact_distance(o, h, p[:-1], q)
    with pytest.raises(ValueError):
        cp.contact_distance(o, h, p, torch.ones(5, 1))
    with pytest.raises(ValueError):
        cp.contact_distance(torch.zeros(7, 2), h, p, q)
    with pytest.raises(ValueError):
        cp.contact_distance(o.double(), h, p, q)
    with pytest.raises(ValueError):
        cp.contact_distance(o, h, p.half(), q)
    with pytest.raises(ValueError):
        cp.contact_distance(torch.zeros(2, 7, 3), torch.zeros(3, 5, 3), p, q)
    with pytest.raises(ValueError):
        cp.contact_distance([[0.0, 0.0, 0.0]], h, p, q)
    with pytest.raises(ValueError):
        cp.contact_agreement({"pred_contact_3d": None}, {"pred_contact_3d": p}, h, o)
