"""The cases of tests/test_screen_bits_gpu.py and tests/golden/make_golden_screen_bits.py: every output of the two files that walk
the faces of a posed mesh in screen space - csrc/silhouette.hip (soft silhouette, its image terms) and csrc/depth_order.hip (z-buffer,
depth-order term) - and of their callers in the fit, on inputs chosen for where a shared walk can go wrong: tile tails, several
256-face chunks per tile, an empty union box, skipped faces, a box of more pixels than one fp32 chain holds, a pose inside a batch.
A case is a function of the device that returns a list of tensors; ``record`` turns it into strings that compare equal exactly when
every bit does (``_lift_bits.encode``).

All inputs come from the CPU references of the tests beside this file, or from seeded CPU generators.
"""
import functools

import numpy as np
import torch

import _depth_order_ref as dref
import _silhouette_ref as sref
from _lift_bits import encode
from interactvlm_amd import fit, occlusion
from interactvlm_amd import silhouette as sil

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _words(t):
    """fp64 values as pairs of int32 words, which ``encode`` takes"""
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float64 else t


def record(name, dev):
    with torch.enable_grad():  # (a test module elsewhere in the suite may have switched autograd off for the process)
        return [f"{tuple(t.shape)} {encode(_words(t))}" for t in CASES[name](dev)]


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _alpha_and_gradient(dev, verts, faces, cam, sigma, blur, g):
    """-> [alpha, d sum(g alpha) / d verts]; g: an image per pose, or the seed of a normal one"""
    v = verts.to(dev).clone().requires_grad_(True)
    a = sil.soft_silhouette(v, faces.to(dev), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), sigma, blur)
    g = _randn(tuple(a.shape), g) if isinstance(g, int) else g
    (gv,) = torch.autograd.grad(a, v, g.to(dev))
    return [a.detach(), gv]


@case
def silhouette_tile_tails(dev):
    """the 6 x 8 sphere at 24 x 40: with 16-pixel tiles both sides end in a partial tile.  sigma 1e-4 with the default blur grows the
    boxes by 0.36 pixels (next to nothing), sigma 4e-3 with blur 3 sigma by 1.3"""
    verts, faces, cam = sref.scene(6, 8, 24, 40)
    return (_alpha_and_gradient(dev, verts, faces, cam, 1e-4, None, 0)
            + _alpha_and_gradient(dev, verts, faces, cam, 4e-3, 3 * 4e-3, 1))


@case
def silhouette_six_chunks(dev):
    """the 24 x 32 sphere at 40 x 56: 1472 faces are six 256-face chunks per tile, the last one partial; faces smaller than a pixel"""
    verts, faces, cam = sref.scene(24, 32, 40, 56)
    assert faces.shape[0] == 1472
    return _alpha_and_gradient(dev, verts, faces, cam, 1e-3, None, 2)


@case
def silhouette_batch(dev):
    """B = 3 with one topology: pose 0 is the scene of silhouette_tile_tails, pose 1 is wholly off-screen (an empty union box: every
    tile leaves early), pose 2 stands across the camera plane (vertices at Z <= 1e-6: their faces are skipped).  Then pose 0 in a call
    of its own: outputs 2 and 3 equal row 0 of outputs 0 and 1, which the test asserts."""
    verts, faces, cam = sref.scene(6, 8, 24, 40)
    poses = torch.stack([verts, verts + torch.tensor([100.0, 0.0, 0.0]), verts + torch.tensor([0.0, 0.0, -2.8])])
    assert bool((poses[2, :, 2] <= 1e-6).any()) and bool((poses[2, :, 2] > 1e-6).any())
    sigma, g = 4e-3, _randn((3, cam.H, cam.W), 3)
    return _alpha_and_gradient(dev, poses, faces, cam, sigma, 3 * sigma, g) + _alpha_and_gradient(dev, poses[0], faces, cam, sigma, 3 * sigma, g[0])


def _unproject(uv, cam, z):
    uv, z = torch.tensor(uv, dtype=torch.float64), torch.tensor(z, dtype=torch.float64)
    return torch.stack(((uv[:, 0] - cam.px) * z / cam.fx, (uv[:, 1] - cam.py) * z / cam.fy, z), -1).float()


@case
def one_triangle_larger_than_the_image(dev):
    """one face whose box is the whole 48 x 64 image, two vertices off-screen and two edges across the image: 3072 pixels are 48 per
    lane of the one wave that walks them - one full fp32 chain of 32 and a partial one of 16 - in both backward kernels"""
    cam = sref.camera(48, 64)
    verts = _unproject([(-50.0, -25.0), (120.0, 18.0), (24.0, 47.5)], cam, [2.0, 3.0, 4.0])
    faces = torch.tensor([[0, 1, 2]])
    sigma = 4e-3
    out = _alpha_and_gradient(dev, verts, faces, cam, sigma, 3 * sigma, 4)
    pv, pf = dref.plane(3.0)
    camera = (cam.fx, cam.fy, cam.px, cam.py)
    occ = torch.as_tensor(dref.depth_image(pv, pf, camera, cam.H, cam.W)[0].astype(np.float32)).to(dev)
    c = torch.as_tensor(dref.weight_image(cam.H, cam.W)).to(dev)
    v = verts.to(dev).clone().requires_grad_(True)
    L = occlusion.depth_order(v, faces.to(dev), occ, c, camera[:2], camera[2:], 0.05)
    (gv,) = torch.autograd.grad(L, v, torch.tensor([0.7], device=dev))
    d, k = occlusion.depth_image(verts.to(dev), faces.to(dev), camera[:2], camera[2:], (cam.H, cam.W))
    assert int((k == 0).sum()) > 64 * 32 and bool((gv != 0).any())
    return out + [d, k, L.detach(), gv]


@case
def silhouette_terms(dev):
    """loss, centroid, the five fp64 sums and the d / d alpha image at 33 x 70 (one row is not a multiple of anything) and 1 x 1, B = 2,
    once with one target shared by the batch and once with a target per pose"""
    out = []
    for H, W in ((33, 70), (1, 1)):
        gen = torch.Generator().manual_seed(11)
        alpha = torch.rand(H, W, generator=gen)
        target = (torch.rand(H, W, generator=gen) < 0.4).float()
        for t in (target[None], torch.stack((target, 1.0 - target))):
            a = torch.stack((alpha, alpha.flip(0) * 0.5)).to(dev).requires_grad_(True)
            loss, centroid, sums = sil._SilhouetteTerms.apply(a, t.to(dev).contiguous())
            (ga,) = torch.autograd.grad([loss, centroid], a, [torch.tensor([0.7, -0.2], device=dev),
                                                              torch.tensor([[-1.3, 0.45], [0.6, 1.1]], device=dev)])
            out += [loss.detach(), centroid.detach(), sums, ga]
    return out


def _depth(dev, v, f, cam, H, W):
    return list(occlusion.depth_image(torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev), cam[:2], cam[2:], (H, W)))


@case
def depth_image(dev):
    """the z-buffer and the winners on the two scenes of tests/test_depth_order_gpu.py (24 x 40 with 80 faces, 48 x 64 with 1472), and
    the small one with every face listed twice (equal depths: the lower index wins)"""
    out = []
    for which in (dref.SMALL, dref.LARGE):
        v, f, cam, H, W = dref.scene(which)
        out += _depth(dev, v, f, cam, H, W)
    v, f, cam, H, W = dref.scene(dref.SMALL)
    return out + _depth(dev, v, np.concatenate([f, f]), cam, H, W)


@functools.lru_cache(maxsize=None)
def _straddle_soft():
    return dref.order_case("straddle_soft")


@case
def depth_order(dev):
    """value and vertex gradient of the straddle_soft case: one pose, then three poses shifted in Z (in front of, across and behind
    the occluder's plane in other proportions)"""
    k = _straddle_soft()
    f = torch.as_tensor(k["faces"]).to(dev)
    occ, c = torch.as_tensor(k["occ"]).to(dev), torch.as_tensor(k["c"]).to(dev)
    cam = k["cam"]
    v0 = torch.as_tensor(k["verts"])
    out = []
    for poses, g in ((v0[None], [0.7]), (torch.stack([v0, v0 + torch.tensor([0.0, 0.0, 0.11]), v0 + torch.tensor([0.0, 0.0, -0.2])]), [0.7, -1.3, 2.0])):
        v = poses.to(dev).clone().requires_grad_(True)
        L = occlusion.depth_order(v, f, occ, c, cam[:2], cam[2:], k["tau"])
        (gv,) = torch.autograd.grad(L, v, torch.tensor(g, device=dev))
        assert bool((gv != 0).any())
        out += [L.detach(), gv]
    return out


@case
def device_pose_fit(dev):
    """fit_step.hip is not one of the two files, but it calls the silhouette's entry points on its own workspace: four iterations of
    fit.DevicePoseFit on the scene of tests/test_fit_device_gpu.py (the 12 x 16 sphere at 64 x 64, two starts, a centroid offset) ->
    parameters, moments, last gradients, counter and both histories"""
    import test_silhouette_gpu as tsg

    cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = tsg.fit_scene()
    scene = (obj.to(dev), faces.to(dev), hum.to(dev), p_obj.to(dev), p_hum.to(dev), target.to(dev), (cam.fx, cam.fy), (cam.px, cam.py))
    dfit = fit.DevicePoseFit(R6.to(dev), T.to(dev), 1.0, *scene, offset.to(dev), max_iter=4).run()
    assert dfit.iteration == 4
    return [t.detach() for t in dfit._state()]


@case
def object_pose_fit_with_occlusion(dev):
    """one forward and backward of fit.ObjectPoseFit(occlusion=True) with depth_order_loss configured, on the scene of
    tests/test_fit_occlusion_gpu.py, from two starts (the cube behind the body and in front of it) -> total, the four terms, the
    gradients of the rotation and the translation"""
    import test_fit_occlusion_gpu as tfo

    args, offset, hf = tfo.scene(dev)
    r6 = torch.tensor(tfo.ir.IDENTITY6, device=dev).repeat(2, 1)
    t = torch.tensor([tfo.TRUE, tfo.FRONT], device=dev)
    model = fit.ObjectPoseFit(r6, t, 1.0, *args, offset, human_faces=hf, occlusion=True)
    total, terms = model(tfo.with_do())
    total.sum().backward()
    assert set(terms) == {"mask_loss", "centroid_loss", "contact_loss", tfo.DO}
    return [total.detach()] + [terms[k].detach() for k in sorted(terms)] + [model.rotation.grad, model.translation.grad]
