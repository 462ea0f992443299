"""The device-resident fit loop on the GPU: ivlm_fit_adam against fit.adam_reference (fp64), iteration 0 of fit.DevicePoseFit against
the torch step of ObjectPoseFit(fused_transform=True) bit for bit, the phases of a run, determinism (repeats, a poisoned
workspace, batch against single starts, chunks), the multi-start search against the fp64 fixture tests/golden/pose_search_fp64.json,
memory and the refusals of the C entry points."""
import ctypes
import functools
import itertools
import json
import os

import pytest
import torch

import _pose_scene as ps
import _silhouette_ref as ref
import test_pose_gpu as tpg
import test_silhouette_gpu as tsg
from interactvlm_amd import _lib, fit, pose
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def grad_enabled():
    with torch.enable_grad():
        yield


# ---- Adam alone -----------------------------------------------------------------------------------------------------------------

GROUPS = (("rotation", 6, 5e-2, "pose"), ("translation", 3, 1e-2, "pose"), ("scale", 1, 1e-2, "scale"))


def _within_one_ulp(got, want64):
    """got (fp32) is the fp64 result rounded to fp32, or one of that value's two fp32 neighbours"""
    want = want64.float()
    inf = torch.full_like(want, float("inf"))
    return bool(((got == want) | (got == torch.nextafter(want, inf)) | (got == torch.nextafter(want, -inf))).all())


@pytest.mark.parametrize("B", [1, 3, 26, 300])  # 26 x 10 elements cross one 256-thread block
def test_adam_against_the_fp64_reference(hip_lib, cuda, B):
    gen = torch.Generator().manual_seed(B)
    stream = torch.cuda.current_stream().cuda_stream
    for t, vars in itertools.product((1, 2, 1000), (("pose",), ("scale",), ("pose", "scale"))):
        host, dev = {}, {}
        for name, n, _, _ in GROUPS:
            shape = (B, n) if n > 1 else (B,)
            host[name] = (torch.randn(shape, generator=gen), torch.randn(shape, generator=gen) * 10.0 ** float(torch.randint(-4, 3, (1,), generator=gen)),
                          torch.randn(shape, generator=gen) * 0.1, torch.rand(shape, generator=gen) * 0.01)  # p, g, m, v
            dev[name] = [x.to(cuda) for x in host[name]]
        counter = torch.tensor([t - 1], dtype=torch.int32, device=cuda)
        ptr = lambda k: [dev[name][k].data_ptr() if (k != 1 or var in vars) else None for name, _, _, var in GROUPS]  # noqa: E731
        rc = hip_lib.ivlm_fit_adam(*ptr(0), *ptr(1), *ptr(2), *ptr(3), B, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 0.9, 0.999, 1e-8, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(counter) == t - 1  # read, not advanced
        for name, _, lr, var in GROUPS:
            p, g, m, v = host[name]
            if var not in vars:  # a NULL gradient: the group is bit-unchanged
                assert all(torch.equal(d.cpu(), h) for d, h in zip(dev[name], host[name])), f"{name} changed without a gradient"
                continue
            for got, want, what in zip((dev[name][0], dev[name][2], dev[name][3]), fit.adam_reference(p, g, m, v, t, lr), "pmv"):
                assert _within_one_ulp(got.cpu(), want), f"{name} {what} at t={t}, B={B}: more than 1 ulp from the fp64 result"
            assert torch.equal(dev[name][1].cpu(), g)


def test_adam_zero_gradient_and_refusals(hip_lib, cuda):
    B = 5
    stream = torch.cuda.current_stream().cuda_stream
    p = [torch.randn(B, 6, device=cuda), torch.randn(B, 3, device=cuda), torch.randn(B, device=cuda)]
    p[0][0, 0], p[1][0, 0] = 0.0, -0.0
    before = [x.clone() for x in p]
    zeros = lambda: [torch.zeros(B, 6, device=cuda), torch.zeros(B, 3, device=cuda), torch.zeros(B, device=cuda)]  # noqa: E731
    g, m, v = zeros(), zeros(), zeros()
    counter = torch.zeros(1, dtype=torch.int32, device=cuda)
    ptrs = lambda xs: [x.data_ptr() for x in xs]  # noqa: E731
    assert hip_lib.ivlm_fit_adam(*ptrs(p), *ptrs(g), *ptrs(m), *ptrs(v), B, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 0.9, 0.999, 1e-8, stream) == 0
    torch.cuda.synchronize()
    for a, b in zip(p, before):  # g = 0 with m = v = 0: the parameter keeps its bits (signed zeros included)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not any(bool(x.any()) for x in m + v)
    # nothing to do, no counter, a bad beta: refused before any launch
    assert hip_lib.ivlm_fit_adam(*ptrs(p), None, None, None, *ptrs(m), *ptrs(v), B, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 0.9, 0.999, 1e-8, stream) == -1
    assert hip_lib.ivlm_fit_adam(*ptrs(p), *ptrs(g), *ptrs(m), *ptrs(v), B, None, 5e-2, 1e-2, 1e-2, 0.9, 0.999, 1e-8, stream) == -1
    assert hip_lib.ivlm_fit_adam(*ptrs(p), *ptrs(g), *ptrs(m), *ptrs(v), B, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 1.0, 0.999, 1e-8, stream) == -1
    assert hip_lib.ivlm_fit_adam(*ptrs(p), *ptrs(g), *ptrs(m), *ptrs(v), B, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 0.9, 0.999, 0.0, stream) == -1
    assert hip_lib.ivlm_fit_adam(*ptrs(p), *ptrs(g), *ptrs(m), *ptrs(v), 65536, counter.data_ptr(), 5e-2, 1e-2, 1e-2, 0.9, 0.999, 1e-8, stream) == -4


# ---- the scenes ------------------------------------------------------------------------------------------------------------------

def _scene_args(cuda, name, sel=None):
    """-> (init R6, T, s), the scene arguments of ObjectPoseFit after them, the centroid offset"""
    if name == "fit":  # test_silhouette_gpu.fit_scene(): B = 2, with a centroid offset
        cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = tsg.fit_scene()
        sel = slice(0, 2) if sel is None else sel
        R6, T, s = R6[sel].to(cuda), T[sel].to(cuda), 1.0
        offset = offset.to(cuda)
    else:  # the search scene: the cube starts ``sel``
        cam, obj, faces, hum, p_obj, p_hum, target, T_start = ps.search_scene()
        sel = [0, 7, 23] if sel is None else sel
        R6, T, s = pose.pose_starts(pose.cube_rotations()[sel].to(cuda), None, T_start.to(cuda), 1.0)
        offset = None
    scene = (obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py))
    return (R6, T, s), scene, offset


def _device_fit(cuda, name, sel=None, **kw):
    init, scene, offset = _scene_args(cuda, name, sel)
    return fit.DevicePoseFit(*init, *scene, offset, **kw)


def _torch_step(cuda, name, vars, weights, step=0):
    init, scene, offset = _scene_args(cuda, name)
    model = fit.ObjectPoseFit(*init, *scene, offset, vars=vars, fused_transform=True)
    total, terms = model(weights, step=step)
    total.sum().backward()
    return model, total.detach(), terms


def _assert_step_equals_torch(dfit, model, total, terms, row=0):
    B = total.shape[0]
    assert torch.equal(dfit.history[row], total), "the total differs from the torch step"
    for k, key in enumerate(fit.TERM_KEYS):
        want = terms[key].detach() if key in terms else torch.zeros(B, device=total.device)
        assert torch.equal(dfit.term_history[row, k], want), f"{key} differs from the torch step"
    for got, param, what in ((dfit.rotation_grad, model.rotation, "rot6d"), (dfit.translation_grad, model.translation, "translation"),
                             (dfit.scale_grad, model.scale, "scale")):
        if param.requires_grad:
            assert torch.equal(got, param.grad), f"d total / d {what} differs from the torch step"
        else:
            assert got is None


@pytest.mark.parametrize("name", ["fit", "search"])
@pytest.mark.parametrize("vars", [("pose",), ("pose", "scale"), ("scale",)])
def test_iteration_0_is_the_torch_step(hip_lib, cuda, name, vars):
    model, total, terms = _torch_step(cuda, name, vars, None)
    assert set(terms) == set(fit.TERM_KEYS) and bool((total > 0).all())
    dfit = _device_fit(cuda, name, vars=vars, max_iter=3)
    start = [x.clone() for x in (dfit.rotation, dfit.translation, dfit.scale)]
    dfit.step()
    assert dfit.iteration == 1 and int(dfit.counter) == 1
    _assert_step_equals_torch(dfit, model, total, terms)
    assert not bool(dfit.history[1:].any()) and not bool(dfit.term_history[1:].any())  # one row per iteration
    # the update is Adam's first step (|delta| = lr up to eps / |g| and rounding) for what is optimised, nothing for the rest
    for k, (now, was, lr, var) in enumerate(zip((dfit.rotation, dfit.translation, dfit.scale), start, fit.DEFAULT_LRS, ("pose", "pose", "scale"))):
        if var not in vars:
            assert torch.equal(now, was)
            continue
        g = dfit._grads[k]
        want, _, _ = fit.adam_reference(was, g, torch.zeros_like(g), torch.zeros_like(g), 1, lr)
        assert _within_one_ulp(now.cpu(), want.cpu())


# ---- phases -----------------------------------------------------------------------------------------------------------------------

PHASED = {"mask_loss": {"w": 5.0, "kick_in": 0}, "centroid_loss": {"w": 1e-4, "kick_in": -1}, "contact_loss": {"w": 10.0, "kick_in": 3}}


def test_phases(hip_lib, cuda):
    dfit = _device_fit(cuda, "fit", loss_weights=PHASED, max_iter=6)
    assert dfit.phases == [(0, 3, 1), (3, 6, 5)]
    dfit.step()
    model, total, terms = _torch_step(cuda, "fit", ("pose",), PHASED)
    assert set(terms) == {"mask_loss"}
    _assert_step_equals_torch(dfit, model, total, terms)  # iteration 0 is the torch step with those weights
    dfit.run()
    assert dfit.iteration == 6 and int(dfit.counter) == 6
    with pytest.raises(RuntimeError, match="iterations have run"):
        dfit.step()
    th, hist = dfit.term_history, dfit.history
    assert bool((th[:3, 2] == 0).all()) and bool((th[3:, 2] > 0).all())
    assert bool((th[:, 1] == 0).all()) and bool((th[:, 0] > 0).all())
    w_m, w_k = torch.tensor(5.0, device=cuda), torch.tensor(10.0, device=cuda)
    want = torch.zeros_like(hist) + th[:, 0] * w_m  # the kernel's order: ((0 + mask w_m) + contact w_k), products rounded first
    want[3:] = want[3:] + th[3:, 2] * w_k
    assert torch.equal(hist, want)
    # iteration 3 is the torch step of the second phase at the parameters the device loop had then
    again = _device_fit(cuda, "fit", loss_weights=PHASED, max_iter=6).run(3)
    init, scene, offset = _scene_args(cuda, "fit")
    model = fit.ObjectPoseFit(again.rotation, again.translation, again.scale, *scene, offset, fused_transform=True)
    total, terms = model(PHASED, step=3)
    total.sum().backward()
    again.step()
    assert set(terms) == {"mask_loss", "contact_loss"}
    _assert_step_equals_torch(again, model, total.detach(), terms, row=3)
    assert torch.equal(again.history[:4], hist[:4])  # and a second run repeats the first across the phase change


def test_contact_only_launches_no_silhouette_kernel(hip_lib, cuda):
    """the project has no launch counter for these kernels: both image terms stay exact zeros, and the run equals one on a 1 x 1
    target mask, which the silhouette kernels would have rendered differently had they run"""
    only = {"contact_loss": {"w": 10.0, "kick_in": 0}}
    dfit = _device_fit(cuda, "fit", loss_weights=only, max_iter=4)
    assert dfit.phases == [(0, 4, 4)]
    dfit.step()
    model, total, terms = _torch_step(cuda, "fit", ("pose",), only)
    _assert_step_equals_torch(dfit, model, total, terms)
    dfit.run()
    assert not bool(dfit.term_history[:, :2].any()) and bool((dfit.term_history[:, 2] > 0).all())
    assert torch.equal(dfit.history, dfit.term_history[:, 2] * torch.tensor(10.0, device=cuda))
    init, scene, offset = _scene_args(cuda, "fit")
    tiny = fit.DevicePoseFit(*init, *scene[:5], torch.ones(1, 1, device=cuda), *scene[6:], offset, loss_weights=only, max_iter=4).run()
    for a, b in zip(dfit._state(), tiny._state()):
        assert torch.equal(a, b)


# ---- determinism --------------------------------------------------------------------------------------------------------------------

def _bits_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a._state(), b._state()))


def test_repeats(hip_lib, cuda):
    runs = [_device_fit(cuda, "fit", max_iter=20).run() for _ in range(2)]
    runs[1].workspace.fill_(255)  # nothing is carried in the workspace from one iteration to the next, or read before it is written
    again = _device_fit(cuda, "fit", max_iter=20)
    again.workspace.fill_(255)
    assert _bits_equal(runs[0], runs[1]), "two runs differ"
    assert _bits_equal(runs[0], again.run()), "a run on a poisoned workspace differs"
    assert int(runs[0].counter) == 20 and bool(torch.isfinite(runs[0].history).all())
    assert float(runs[0].history[-1].max()) < float(runs[0].history[0].min())  # and it descends
    out = runs[0].result()
    assert out["history"].shape == (20, 2) and out["term_history"].shape == (20, 3, 2) and out["object_vertices"].shape[0] == 2


@functools.lru_cache(maxsize=None)
def _all_starts(cuda):
    """the 24 cube starts of the search scene in one device loop, run once and shared (never modified)"""
    return _device_fit(cuda, "search", sel=list(range(24)), max_iter=ps.MAX_ITER).run()


@pytest.mark.parametrize("k", [0, 7, 23])
def test_start_equals_its_own_run(hip_lib, cuda, k):
    batch, own = _all_starts(cuda), _device_fit(cuda, "search", sel=[k], max_iter=ps.MAX_ITER).run()
    assert torch.equal(own.history[:, 0], batch.history[:, k]) and torch.equal(own.term_history[:, :, 0], batch.term_history[:, :, k])
    for a, b in zip(own._state()[:12], batch._state()[:12]):  # parameters, moments, last gradients
        assert torch.equal(a[0], b[k])


def _search(cuda, **kw):
    return tpg._search(cuda, rotations=None, icp=False, device_loop=True, **kw)


@functools.lru_cache(maxsize=None)
def _search_all(cuda):
    return _search(cuda)


def test_search_chunk_changes_no_bit(hip_lib, cuda):
    res, chunked = _search_all(cuda), _search(cuda, chunk=5)
    for k in ("rotation", "translation", "scale", "object_vertices", "history", "term_history", "scores", "best_index"):
        assert torch.equal(res[k], chunked[k]), f"{k} differs with chunk=5"
    assert torch.equal(res["history"], _all_starts(cuda).history)  # and fit_object_pose(device_loop=True) is DevicePoseFit.run()


# ---- the search ---------------------------------------------------------------------------------------------------------------------

def test_search_finds_the_fp64_winner_as_closely_as_the_torch_loop(hip_lib, cuda):
    """The scores of the device loop against the fp64 finals of the fixture, beside those of the torch loop: the two loops share
    every loss and gradient kernel and differ in Adam's rounding alone, so their distances to fp64 are set by the shared kernels;
    a factor of 2 is the margin for what 20 iterations amplify.  The maximum is over all 24 starts; both figures are printed."""
    res = _search_all(cuda)
    scores = res["scores"]
    assert res["history"].shape == (ps.MAX_ITER, 24) and res["term_history"].shape == (ps.MAX_ITER, 3, 24)
    assert int(res["best_index"]) == 7
    assert float(scores[0] - scores[7]) > 1.0
    assert bool(torch.isfinite(scores).all())
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ps.GOLDEN)) as f:
        gold = torch.tensor(json.load(f)["final_total"], dtype=torch.float64)
    e_dev = float((scores.double().cpu() - gold).abs().max())
    e_torch = float((tpg._search_all(cuda)["scores"].double().cpu() - gold).abs().max())
    print(f"max |score - fp64| over the 24 starts: device loop {e_dev:.3e}, torch loop {e_torch:.3e}")
    assert e_dev <= 2 * e_torch


# ---- memory and refusals ------------------------------------------------------------------------------------------------------------

def test_run_does_not_allocate(hip_lib, cuda):
    B, H, W, N_h = 24, 512, 512, 431
    obj, faces = ref.uv_sphere(33, 64)
    N, F = obj.shape[0], faces.shape[0]
    assert (N, F) == (2050, 4096)
    gen = torch.Generator().manual_seed(1)
    hum = (torch.randn(N_h, 3, generator=gen) * 0.3 + torch.tensor([0.9, 0.0, 3.0])).to(cuda)
    p_obj, p_hum = (torch.rand(N, generator=gen) < 0.05).float().to(cuda), (torch.rand(N_h, generator=gen) < 0.1).float().to(cuda)
    target = torch.zeros(H, W, device=cuda)
    target[180:330, 190:340] = 1.0
    T = torch.tensor([0.1, -0.05, 3.0]) + torch.arange(B)[:, None] * torch.tensor([0.01, 0.0, 0.02])
    dfit = fit.DevicePoseFit(fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(cuda), T.to(cuda), 1.0, obj.float().to(cuda), faces.to(cuda),
                             hum, p_obj, p_hum, target, (1.5 * W, 1.5 * W), (W / 2 + 1.3, H / 2 - 0.7), max_iter=4)
    ws = hip_lib.ivlm_fit_step_workspace_bytes(B, N, F, H, W, N_h)
    assert dfit.workspace.numel() == ws > 0
    dfit.step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dfit.run()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    state = sum(t.numel() * t.element_size() for t in dfit._state())
    print(f"peak memory rise of run() {rise / 1e6:.3f} MB; workspace {ws / 1e6:.2f} MB, state and histories {state / 1e3:.1f} kB")
    assert rise <= ws + state + (1 << 20)  # the issue's bound
    assert rise <= (1 << 20)               # and what holds: all of that was allocated by the constructor
    assert dfit.iteration == 4 and bool(torch.isfinite(dfit.history).all())


def test_device_refusals(hip_lib, cuda):
    dfit = _device_fit(cuda, "search", max_iter=2)
    stream = torch.cuda.current_stream().cuda_stream
    good = _lib.FitStepArgs.from_buffer_copy(dfit._args)
    good.terms_on = 7

    def call(**change):
        a = _lib.FitStepArgs.from_buffer_copy(good)
        for k, v in change.items():
            setattr(a, k, v)
        return hip_lib.ivlm_fit_step(ctypes.byref(a), stream)

    before = [t.clone() for t in dfit._state()]
    assert call(N=(1 << 22) + 1) == -4 and call(B=65536) == -4 and call(H=16385) == -4 and call(N_h=(1 << 20) + 1) == -4
    assert call(sigma=0.0) == -4 and call(p_dtype=5) == -4
    assert call(terms_on=0) == -1 and call(terms_on=8) == -1 and call(optimise=0) == -1 and call(step=None) == -1 and call(max_iter=0) == -1
    assert call(grad_rotation=None) == -1 and call(beta1=1.0) == -1 and call(eps=0.0) == -1
    assert call(workspace_bytes=good.workspace_bytes - 1) == -2 and call(workspace=good.workspace + 16) == -2
    assert hip_lib.ivlm_fit_step(None, stream) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dfit._state(), before)), "a refused call launched something"
    assert call() == 0  # and the unchanged arguments run
    torch.cuda.synchronize()
    assert int(dfit.counter) == 1 and bool((dfit.history[0] > 0).all())
    with pytest.raises(ValueError, match="n: expected"):
        dfit.run(5)
    # sizes a member refuses are refused by the constructor, before any launch
    init, scene, offset = _scene_args(cuda, "search")
    with pytest.raises(IvlmError, match="not supported"):
        fit.DevicePoseFit(*init, *scene[:5], torch.ones(16385, 2, device=cuda), *scene[6:], offset)
