"""The intrusion term in the object-pose fit (fit.ObjectPoseFit / fit_object_pose / search_object_pose with intrusion=True).

The scene of the issue: the human is ``body_mesh(12, 11)`` at the origin (134 vertices), the object an 8-vertex cube of half 0.2 placed
at (0.05, 0.78, 0.03) by the translation, identity rotation, s = 1, a 32 x 32 target mask, human_faces given.  None of the cube's 8
vertices lies inside the body - ``penetration_loss`` is an exact 0 - while 25 of the body's vertices lie inside the cube: the fp64
reference (tests/_intrusion_ref.py) gives L = 1.6228e-3 there, unique closest points, the nearest point 5.1e-3 from the surface.
Tolerances are those of tests/test_intrusion_gpu.py (K 2^-24 scale, the constants measured on the CPU).

The descent: the term alone, rotation and translation free, the reference's learning rates, 80 iterations; the last 20 totals are
exactly 0.  An fp64 Adam simulation on the CPU reaches an exact 0 at iteration 49 and stays there (the object keeps drifting away
on Adam's momentum); the GPU's fp32 trajectory arrived at iteration 49 as well (printed by the test).
"""
import numpy as np
import pytest
import torch

import _intrusion_ref as ir
from interactvlm_amd import fit
from interactvlm_amd.pose import cube_rotations
from test_intrusion_gpu import K_L, K_R, K_T

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INT, PEN = "intrusion_loss", "penetration_loss"
ONLY_INT = {INT: {"w": 1.0, "kick_in": 0}}
FOCAL, PRINCIPAL = (48.0, 48.0), (17.3, 15.3)


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


def scene(dev):
    """-> (the eight positional scene arguments, offset, human_faces), on dev"""
    hv, hf, cv, cf = (torch.from_numpy(a) for a in ir.fit_scene())
    p_obj = (cv[:, 1] < 0).float() * 0.8
    p_hum = (hv[:, 1] > 0.5).float() * 0.6
    target = torch.zeros(32, 32)
    target[13:19, 14:20] = 1.0
    offset = torch.tensor([0.0, -0.78, 3.0])
    args = tuple(t.to(dev) for t in (cv, cf, hv, p_obj, p_hum, target)) + (FOCAL, PRINCIPAL)
    return args, offset.to(dev), hf.to(dev)


def start(dev, B=1):
    return (torch.tensor(ir.IDENTITY6, device=dev).repeat(B, 1), torch.tensor(ir.CUBE_CENTRE, device=dev).repeat(B, 1), 1.0)


def with_int(kick_in=0, w=3.0):
    return {**fit.DEFAULT_LOSS_WEIGHTS, INT: {"w": w, "kick_in": kick_in}}


def reference():
    hv, _, cv, cf = ir.fit_scene()
    return ir.intrusion(hv, ir.IDENTITY6, np.array(ir.CUBE_CENTRE, dtype=np.float32), 1.0, cv, cf, unique=True)


def test_penetration_sees_nothing_where_intrusion_sees_the_limb(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda), *args, offset, human_faces=hf, intrusion=True)
    with torch.no_grad():
        _, terms = model({PEN: {"w": 1.0, "kick_in": 0}, INT: {"w": 1.0, "kick_in": 0}})
    w = reference()
    assert int(w["inside"].sum()) == 25 and w["r"]["unique"][w["inside"]].all() and abs(w["L"] - 1.6228e-3) < 1e-7
    got = float(terms[INT][0])
    print(f"penetration {float(terms[PEN][0])!r}, intrusion {got:.6e} (fp64 {w['L']:.6e}), |error| {abs(got - w['L']):.2e} <= {K_L * U * w['A']:.2e}")
    assert float(terms[PEN][0]) == 0.0
    assert abs(got - w["L"]) <= K_L * U * w["A"]


def test_term_alone(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda), *args, offset, intrusion=True)
    total, terms = model(ONLY_INT)
    assert set(terms) == {INT} and total.shape == (1,)
    with torch.no_grad():
        direct = model.object_sdf.intrusion(args[2], model.rotation, model.translation, model.scale)
    assert torch.equal(total, terms[INT]) and torch.equal(total, direct) and float(total.detach()) > 0
    total.sum().backward()
    w = reference()
    got = {"L": float(total.detach()), "g_t": model.translation.grad[0].cpu().numpy(), "g_r6": model.rotation.grad[0].cpu().numpy(),
           "g_s": w["g_s"]}  # (the scale is not a variable of this fit)
    c = ir.compare(got, w)  # a component whose scale is 0 - a stretch of a1 at the identity - must be an exact 0
    print(f"ratios against fp64: L {c['L']:.1f} (<= {K_L}), translation {c['t']:.1f} (<= {K_T}), rot6d {c['r']:.1f} (<= {K_R})")
    assert c["L"] <= K_L and c["t"] <= K_T and c["r"] <= K_R
    assert bool((model.rotation.grad != 0).any()) and bool((model.translation.grad != 0).any())


def test_default_weights_give_the_same_bits_with_and_without_intrusion(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    out = []
    for flag in (False, True):
        model = fit.ObjectPoseFit(*start(cuda, 2), *args, offset, human_faces=hf, intrusion=flag)
        total, terms = model()
        total.sum().backward()
        out.append((total.detach(), terms, model.rotation.grad, model.translation.grad))
    (t0, terms0, gr0, gt0), (t1, terms1, gr1, gt1) = out
    assert set(terms0) == set(terms1) == {"mask_loss", "centroid_loss", "contact_loss"}
    assert torch.equal(t0, t1) and torch.equal(gr0, gr1) and torch.equal(gt0, gt1)
    assert all(torch.equal(terms0[k], terms1[k]) for k in terms0)
    # ... and with the key present but switched off
    model = fit.ObjectPoseFit(*start(cuda, 2), *args, offset, human_faces=hf, intrusion=True)
    total, terms = model(with_int(kick_in=-1))
    assert INT not in terms and torch.equal(total, t0)


def test_kick_in(hip_lib, cuda):
    args, offset, _ = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda), *args, offset, intrusion=True)
    weights = with_int(kick_in=2)
    seen = []
    with torch.no_grad():
        for _ in range(3):
            total, terms = model(weights)
            seen.append(INT in terms)
    assert seen == [False, False, True] and model.step == 3
    rest = ((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0
    assert torch.equal(total, rest + terms[INT] * 3.0) and float(terms[INT]) > 0


def test_term_on_without_intrusion_raises(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda), *args, offset, human_faces=hf)
    with pytest.raises(ValueError, match="intrusion"):
        model(ONLY_INT)
    model(with_int(kick_in=-1))  # configured but off: nothing to refuse
    with pytest.raises(ValueError, match="intrusion"):
        fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, loss_weights=ONLY_INT, max_iter=2)
    # an object that is not closed is refused by the constructor, by name
    with pytest.raises(ValueError, match="no reverse"):
        fit.ObjectPoseFit(*start(cuda), args[0], args[1][:-1], *args[2:], offset, intrusion=True)


def test_device_loop_refuses_the_term(hip_lib, cuda):
    args, offset, _ = scene(cuda)
    with pytest.raises(ValueError, match=INT):
        fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, loss_weights=with_int(), max_iter=2, device_loop=True,
                            intrusion=True)
    with pytest.raises(ValueError, match=INT):
        fit.search_object_pose(*args, rotations=cube_rotations()[:2], icp=False, device_loop=True, intrusion=True,
                               hum_centroid_offset=offset, loss_weights=with_int(), max_iter=2)
    with pytest.raises(ValueError, match=INT):  # and the class itself, which would otherwise leave the term out silently
        fit.DevicePoseFit(*start(cuda), *args, offset, loss_weights=with_int(), max_iter=2)
    # switched off, the device loop runs as before
    out = fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, loss_weights=with_int(kick_in=-1), max_iter=2,
                              device_loop=True, intrusion=True)
    assert out["history"].shape == (2, 1)


def test_search_chunking_and_scores(hip_lib, cuda):
    args, offset, _ = scene(cuda)
    weights = with_int()
    T0 = torch.tensor(ir.CUBE_CENTRE, device=cuda)

    def run(chunk):
        return fit.search_object_pose(*args, rotations=cube_rotations()[:5], init=(None, T0, 1.0), icp=False, chunk=chunk, intrusion=True,
                                      hum_centroid_offset=offset, loss_weights=weights, max_iter=3)

    whole, parts = run(None), run(2)
    assert whole["rotation"].shape == (5, 6) and whole["history"].shape == (3, 5) and whole["scores"].shape == (5,)
    for k, v in whole.items():
        if isinstance(v, dict):
            assert all(torch.equal(v[j], parts[k][j]) for j in v), k
        else:
            assert torch.equal(v, parts[k]), k
    final = fit.ObjectPoseFit(whole["rotation"], whole["translation"], whole["scale"], *args, offset, fused_transform=True, intrusion=True)
    with torch.no_grad():
        total, terms = final(weights, step=0)
    assert set(terms) == {"mask_loss", "centroid_loss", "contact_loss", INT}
    assert torch.equal(whole["scores"], total)
    assert torch.equal(total, (((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0) + terms[INT] * 3.0)
    assert bool((terms[INT] > 0).any())  # the score really holds the term


def test_the_term_alone_pushes_the_limb_out_of_the_object(hip_lib, cuda):
    """only the intrusion term, rotation and translation free, Adam at 5e-2 / 1e-2, 80 iterations from the scene's pose: the last 20
    totals are exactly 0 (fp64 Adam on the CPU: exact 0 from iteration 49 on; 80 is that plus margin for the fp32 trajectory)"""
    args, offset, _ = scene(cuda)
    out = fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, vars=("pose",), loss_weights=ONLY_INT, max_iter=80,
                              intrusion=True)
    history = out["history"][:, 0].tolist()
    first = next((i for i, h in enumerate(history) if h == 0.0), None)
    print("intrusion, first -> last:", history[0], "->", history[-1], "; first exact 0 at iteration", first)
    assert len(history) == 80 and history[0] > 1e-3
    assert all(h == 0.0 for h in history[-20:])
