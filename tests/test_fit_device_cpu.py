"""The device-resident fit loop (fit.DevicePoseFit, csrc/fit_step.hip) without a GPU: the Adam yardstick of the kernel test against
torch.optim.Adam, the phases of a run, the refusals that must come before the library loads, and the header / ctypes declarations."""
import ctypes
import os
import re

import pytest
import torch

from interactvlm_amd import _lib, fit
from interactvlm_amd._lib import IvlmError


@pytest.fixture
def no_library(monkeypatch):
    """validation must raise before anything touches the library"""
    def boom():
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(_lib, "load", boom)


def header_struct_fields(name, path=_lib.HEADER_PATH):
    """the field names of ``typedef struct name { ... } name;`` in the header, in order, with 'p' (pointer) or the C type of each"""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S)
    if m is None:
        raise AssertionError(f"{name} is not declared in ivlm_hip.h")
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.replace("const", " ").strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for item in rest.split(","):
            item = item.strip()
            fields.append((item.lstrip("* "), "p" if item.startswith("*") else ctype))
    return fields


def test_adam_reference_against_torch_adam():
    """three groups with the three learning rates, 20 steps of random gradients, everything fp64: the same formula, so the only
    slack is operation order (torch's lerp, its bias-correction placement) - 1e-12 relative"""
    gen = torch.Generator().manual_seed(0)
    shapes, lrs = ((4, 6), (4, 3), (4,)), fit.DEFAULT_LRS
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)])
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    for t in range(1, 21):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 10.0 ** (t % 5 - 3) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        mine = [fit.adam_reference(p, g, m, v, t, lr) for (p, m, v), g, lr in zip(mine, grads, lrs)]
        for k, (p, (q, m, v)) in enumerate(zip(params, mine)):
            state = opt.state[p]
            for got, want, what in ((q, p.detach(), "p"), (m, state["exp_avg"], "m"), (v, state["exp_avg_sq"], "v")):
                assert got.dtype == torch.float64
                err = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
                assert err <= 1e-12, f"group {k} {what} at step {t}: relative error {err:.3e}"


def test_adam_reference_zero_gradient_keeps_the_parameter():
    p = torch.tensor([0.3, -1.5, 0.0], dtype=torch.float32)
    z = torch.zeros(3)
    q, m, v = fit.adam_reference(p, z, z, z, 1, 5e-2)
    assert torch.equal(q.float(), p) and not bool(m.any()) and not bool(v.any())


def test_phases_from_kick_in():
    w = lambda m, c, k: {"mask_loss": {"w": 1.0, "kick_in": m}, "centroid_loss": {"w": 1.0, "kick_in": c},  # noqa: E731
                         "contact_loss": {"w": 1.0, "kick_in": k}}
    assert fit.TERM_KEYS == ("mask_loss", "centroid_loss", "contact_loss")
    assert (_lib.FIT_MASK, _lib.FIT_CENTROID, _lib.FIT_CONTACT) == (1, 2, 4)
    assert fit.fit_phases(None, 250) == [(0, 250, 7)]
    assert fit.fit_phases(w(0, -1, 3), 6) == [(0, 3, 1), (3, 6, 5)]      # -1 is never on, 0 from the start, k from iteration k
    assert fit.fit_phases(w(2, 4, 6), 10) == [(0, 2, 0), (2, 4, 1), (4, 6, 3), (6, 10, 7)]  # at most four phases
    assert fit.fit_phases(w(0, 5, 5), 10) == [(0, 5, 1), (5, 10, 7)]
    assert fit.fit_phases(w(0, 10, 12), 10) == [(0, 10, 1)]               # a kick-in at or past the end never counts
    assert fit.fit_phases({"contact_loss": {"w": 2.0, "kick_in": 0}}, 4) == [(0, 4, 4)]  # a missing key is off
    for weights, n in ((w(0, -1, 3), 6), (w(2, 4, 6), 10), (None, 3)):  # the phases are ObjectPoseFit's rule, iteration by iteration
        ww = fit.DEFAULT_LOSS_WEIGHTS if weights is None else weights
        for lo, hi, bits in fit.fit_phases(weights, n):
            for i in range(lo, hi):
                want = sum(1 << k for k, key in enumerate(fit.TERM_KEYS) if ww[key]["kick_in"] >= 0 and i >= ww[key]["kick_in"])
                assert bits == want


def _scene():
    v, f, h = torch.rand(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]]), torch.rand(3, 3)
    return v, f, h, torch.ones(5), torch.ones(3), torch.ones(8, 8), 10.0, (4.0, 4.0)


def test_refusals_before_the_library_loads(no_library):
    scene = _scene()
    init = (torch.tensor([[1.0, 0, 0, 1, 0, 0]]), torch.zeros(1, 3), 1.0)
    with pytest.raises(ValueError, match="early_stop"):
        fit.fit_object_pose(*scene, init=init, device_loop=True, early_stop=True)
    with pytest.raises(ValueError, match="fused_transform"):
        fit.fit_object_pose(*scene, init=init, device_loop=True, fused_transform=False)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            fit.fit_object_pose(*scene, init=init, device_loop=True, max_iter=bad)
        with pytest.raises(ValueError, match="max_iter"):
            fit.DevicePoseFit(*init, *scene, max_iter=bad)
    for bad in (("pose", "shape"), ("rotation",)):
        with pytest.raises(ValueError, match="vars"):
            fit.fit_object_pose(*scene, init=init, device_loop=True, vars=bad)
        with pytest.raises(ValueError, match="vars"):
            fit.DevicePoseFit(*init, *scene, vars=bad)
    with pytest.raises(ValueError, match="vars"):
        fit.DevicePoseFit(*init, *scene, vars=())
    with pytest.raises(ValueError, match="no term counts at iteration 0"):
        fit.DevicePoseFit(*init, *scene, loss_weights={"mask_loss": {"w": 1.0, "kick_in": 2}}, max_iter=4)
    with pytest.raises(ValueError, match="learning rates"):
        fit.DevicePoseFit(*init, *scene, lrs=(1e-2, 1e-2))
    with pytest.raises(ValueError, match="betas"):
        fit.DevicePoseFit(*init, *scene, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps > 0"):  # eps == 0 would make a zero gradient on zero moments 0 / 0
        fit.DevicePoseFit(*init, *scene, eps=0.0)
    with pytest.raises(ValueError, match="translation_init"):
        fit.DevicePoseFit(init[0], torch.zeros(2, 3), 1.0, *scene)
    with pytest.raises(IvlmError, match="GPU tensor"):  # everything else in order: there is no CPU fallback
        fit.DevicePoseFit(*init, *scene)
    with pytest.raises(IvlmError, match="GPU tensor"):
        fit.fit_object_pose(*scene, init=init, device_loop=True)
    with pytest.raises(ValueError, match="early_stop"):
        fit.search_object_pose(*scene, device_loop=True, early_stop=True)


def test_header_symbols_and_declarations():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.header_prototypes()
    for name in ("ivlm_fit_step_workspace_bytes", "ivlm_fit_step", "ivlm_fit_adam"):
        assert name in protos, f"{name} is not declared in include/ivlm_hip.h"
        assert hasattr(lib, name), f"libivlm_hip.so does not export {name}"
    assert protos["ivlm_fit_step"][1][0].replace(" ", "") == "constIvlmFitStepArgs*args"
    assert [a.split()[0] for a in protos["ivlm_fit_adam"][1][-7:-1]] == ["double"] * 6 and _lib._to_ctype("double x") is ctypes.c_double
    txt = open(_lib.HEADER_PATH).read()
    for const, value in (("IVLM_FIT_MASK", _lib.FIT_MASK), ("IVLM_FIT_CENTROID", _lib.FIT_CENTROID), ("IVLM_FIT_CONTACT", _lib.FIT_CONTACT),
                         ("IVLM_FIT_POSE", _lib.FIT_POSE), ("IVLM_FIT_SCALE", _lib.FIT_SCALE)):
        assert f"#define {const} {value}\n" in txt, f"{const} of the header and interactvlm_amd._lib differ"
    # the ctypes structure is the header's struct, field for field
    kinds = {"p": ctypes.c_void_p, "size_t": ctypes.c_size_t, "double": ctypes.c_double, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    want = [(name, kinds[kind]) for name, kind in header_struct_fields("IvlmFitStepArgs")]
    assert list(_lib.FitStepArgs._fields_) == want
    assert ctypes.sizeof(_lib.FitStepArgs) == 26 * 8 + 8 + 6 * 8 + 10 * 4 + 9 * 4 + 4  # no padding but the tail's
    # the workspace formula: the members' workspaces and the step's own buffers, each rounded up to 256 bytes
    ws = lib.ivlm_fit_step_workspace_bytes
    ws.restype = ctypes.c_size_t
    for fn in (lib.ivlm_pose_transform_workspace_bytes, lib.ivlm_soft_silhouette_workspace_bytes, lib.ivlm_contact_pair_workspace_bytes):
        fn.restype = ctypes.c_size_t
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    for B, N, F, H, W, N_h in ((1, 5, 2, 8, 8, 3), (24, 2050, 4096, 512, 512, 431), (3, 86, 168, 48, 48, 50)):
        members = (lib.ivlm_pose_transform_workspace_bytes(B, N), lib.ivlm_soft_silhouette_workspace_bytes(B, N, F, H, W), B * H * 40,
                   lib.ivlm_contact_pair_workspace_bytes(B, N, N_h))
        own = 4 * up(12 * B * N) + 2 * up(4 * B * H * W) + up(40 * B) + up(28 * B)
        assert ws(B, N, F, H, W, N_h) == sum(up(m) for m in members) + own
    for bad in ((0, 5, 2, 8, 8, 3), (65536, 5, 2, 8, 8, 3), (1, (1 << 22) + 1, 2, 8, 8, 3), (1, 5, (1 << 22) + 1, 8, 8, 3),
                (1, 5, 2, 16385, 8, 3), (1, 5, 2, 8, 0, 3), (1, 5, 2, 8, 8, (1 << 20) + 1)):
        assert ws(*bad) == 0, bad
