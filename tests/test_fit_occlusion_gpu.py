"""The occlusion-aware image terms and the depth-order term in the object-pose fit (fit.ObjectPoseFit / fit_object_pose /
search_object_pose with occlusion=True).

The scene: the body and the cube of ``tests/_intrusion_ref.fit_scene()`` in the 32 x 32 camera of tests/test_fit_intrusion_gpu.py.  The
cube (half 0.2) stands at (0.1, 0.78, 0.35): behind the body, a part of it sticking out beside it.  In fp64 (tests/_depth_order_ref.py)
it covers 36 pixels, 14 of them visible and 22 hidden by the body; no pixel of the cube is undecided.  The target mask is those
visible pixels.  The body covers 240 pixels, none of which shows the cube in front, so signed_weight is -1 on 240 pixels and 0
elsewhere.  Tolerances are those of tests/test_depth_order_gpu.py (K 2^-24 scale, the constants measured on the CPU).

The don't-care terms: whether the CENTROID term falls with the don't-care image depends on the scene - its target is the centre of the
visible pixels' bounding box, and the body's outline cuts the cube obliquely - so the placement was chosen from the fp64 references
alone (tests/_silhouette_ref.py and tests/_depth_order_ref.py on the CPU), where both terms fall clearly: mask_loss 0.7396 -> 0.5538,
centroid_loss 1.4911 -> 0.3880.  (At (0.15, 0.78, 0.35) the same references give 0.7438 -> 0.5832 and 0.7457 -> 0.9472: there the
mask term falls and the centroid term does not.)

The descent: the term alone from (0.1, 0.78, -0.6) - the cube 0.3 in front of the body -, rotation and translation free, Adam at
5e-2 / 1e-2, 40 iterations.  An fp64 Adam simulation on the CPU with the winners found afresh every iteration: 1.110e-1 at iteration 0,
5.69e-2 at 10, 1.46e-2 at 20, an exact 0 from 32 on; the translation's Z goes from -0.6 to -0.34.
"""
import numpy as np
import pytest
import torch

import _depth_order_ref as ref
import _intrusion_ref as ir
from interactvlm_amd import fit, occlusion
from interactvlm_amd.pose import cube_rotations
from interactvlm_amd.silhouette import silhouette_terms, soft_silhouette
from test_depth_order_gpu import K_G, K_L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DO = "depth_order_loss"
ONLY_DO = {DO: {"w": 1.0, "kick_in": 0}}
FOCAL, PRINCIPAL = (48.0, 48.0), (17.3, 15.3)
CAM = FOCAL + PRINCIPAL
H = W = 32
OFFSET = (0.0, -0.78, 3.0)
TRUE, FRONT, MIRRORED = (0.1, 0.78, 0.35), (0.1, 0.78, -0.6), (0.1, 0.78, -0.35)


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


_visible = []


def visible_mask():
    """the fp64 visible object pixels at the true pose, from both depth images (computed once)"""
    if not _visible:
        hv, hf, cv, cf = ir.fit_scene()
        off = np.array(OFFSET, dtype=np.float32)
        v = (cv + np.array(TRUE, dtype=np.float32) + off).astype(np.float32)
        d_h, _ = ref.depth_image((hv + off).astype(np.float32), hf, CAM, H, W)
        d_o, _ = ref.depth_image(v, cf, CAM, H, W)
        cls = ref.classify(v, cf, CAM, H, W)
        cover = np.isfinite(d_o)
        assert cls.decided.all() and int(cover.sum()) == 36
        both = cover & np.isfinite(d_h)
        with np.errstate(invalid="ignore"):  # (inf - inf where neither mesh covers, not selected)
            assert np.abs(d_o - d_h)[both].min() > 1e-2  # no pixel where the two surfaces all but touch
        vis = cover & ~(d_h < d_o)
        assert int(vis.sum()) == 14
        _visible.append(vis.astype(np.float32))
    return _visible[0]


def scene(dev):
    """-> (the eight positional scene arguments, offset, human_faces), on dev"""
    hv, hf, cv, cf = (torch.from_numpy(a) for a in ir.fit_scene())
    p_obj = (cv[:, 1] < 0).float() * 0.8
    p_hum = (hv[:, 1] > 0.5).float() * 0.6
    target = torch.from_numpy(visible_mask())
    args = tuple(t.to(dev) for t in (cv, cf, hv, p_obj, p_hum, target)) + (FOCAL, PRINCIPAL)
    return args, torch.tensor(OFFSET).to(dev), hf.to(dev)


def start(dev, centre=TRUE, B=1):
    return (torch.tensor(ir.IDENTITY6, device=dev).repeat(B, 1), torch.tensor(centre, device=dev).repeat(B, 1), 1.0)


def with_do(kick_in=0, w=10.0):
    return {**fit.DEFAULT_LOSS_WEIGHTS, DO: {"w": w, "kick_in": kick_in}}


def test_dont_care_terms_at_the_true_pose(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    plain = fit.ObjectPoseFit(*start(cuda), *args, offset, human_faces=hf)
    aware = fit.ObjectPoseFit(*start(cuda), *args, offset, human_faces=hf, occlusion=True)
    with torch.no_grad():
        _, t0 = plain()
        _, t1 = aware()
        valid = aware.scene.valid
        assert aware.valid is valid and dict(aware.named_buffers())["valid"] is valid and plain.valid is None  # a buffer: .to() moves it
        assert valid.shape == (H, W) and torch.equal(aware.target_mask * valid, aware.target_mask)
        assert int((aware.scene.signed_weight < 0).sum()) == int((valid == 0).sum()) > 0
        alpha = soft_silhouette(aware.object_vertices() + offset, args[1], FOCAL, PRINCIPAL, (H, W), aware.sigma, aware.blur_radius)
        mask_loss, centroid = silhouette_terms(alpha * valid, aware.target_mask)
    d = centroid - aware.target_mask_centroid
    print(f"mask_loss {float(t0['mask_loss']):.4f} -> {float(t1['mask_loss']):.4f} with the don't-care image; centroid_loss "
          f"{float(t0['centroid_loss']):.4f} -> {float(t1['centroid_loss']):.4f}")
    assert float(t1["mask_loss"]) < float(t0["mask_loss"])
    assert torch.equal(t1["mask_loss"], mask_loss)
    assert torch.equal(t1["centroid_loss"], d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    assert float(t1["centroid_loss"]) < float(t0["centroid_loss"])
    assert torch.equal(t0["contact_loss"], t1["contact_loss"])
    # the gradient flows through the multiply
    total, _ = aware(step=0)
    total.sum().backward()
    assert bool((aware.translation.grad != 0).any())


def test_default_weights_give_the_same_bits_without_occlusion(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    out = []
    for kwargs in ({}, {"occlusion": False, "human_mask": None, "depth_tau": 0.01}):
        model = fit.ObjectPoseFit(*start(cuda, B=2), *args, offset, human_faces=hf, **kwargs)
        total, terms = model()
        total.sum().backward()
        out.append((total.detach(), terms, model.rotation.grad, model.translation.grad))
    (t0, terms0, gr0, gt0), (t1, terms1, gr1, gt1) = out
    assert set(terms0) == set(terms1) == {"mask_loss", "centroid_loss", "contact_loss"}
    assert torch.equal(t0, t1) and torch.equal(gr0, gr1) and torch.equal(gt0, gt1)
    assert all(torch.equal(terms0[k], terms1[k]) for k in terms0)
    # ... and with the key present but switched off
    model = fit.ObjectPoseFit(*start(cuda, B=2), *args, offset, human_faces=hf)
    total, terms = model(with_do(kick_in=-1))
    assert DO not in terms and torch.equal(total, t0)


def test_term_at_step_0_against_fp64(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda, FRONT), *args, offset, human_faces=hf, occlusion=True)
    total, terms = model(ONLY_DO)
    assert set(terms) == {DO} and total.shape == (1,) and torch.equal(total, terms[DO] * 1.0)
    with torch.no_grad():
        v = model.object_vertices() + offset
        direct = occlusion.depth_order(v, args[1], model.scene.occluder_depth, model.scene.signed_weight, FOCAL, PRINCIPAL, 0.01)
    assert torch.equal(direct, terms[DO].detach())
    total.sum().backward()
    # the fp64 restatement on the very inputs of the kernel: the fp32 vertices, the scene's occluder depth and signed weights
    v32, occ, c = v[0].cpu().numpy(), model.scene.occluder_depth.cpu().numpy(), model.scene.signed_weight.cpu().numpy()
    cf = args[1].cpu().numpy()
    cls = ref.classify(v32, cf, CAM, H, W)
    assert cls.decided[c != 0].all()
    want = ref.depth_order(v32, cf, np.where(cls.decided, cls.winner, -1), CAM, H, W, occ, c, 0.01)
    got = float(total.detach())
    err_t = np.abs(model.translation.grad[0].cpu().numpy() - want["g"][0].sum(0))
    print(f"step 0: {got:.6e} (fp64 {want['L']:.6e}), |error| {abs(got - want['L']):.2e} <= {K_L * U * want['A']:.2e}; translation gradient "
          f"error / allowance {(err_t / (K_G * U * want['s'][0].sum(0))).max():.4f}")
    assert want["L"] > 1e-2 and abs(got - want["L"]) <= K_L * U * want["A"]
    assert (err_t <= K_G * U * want["s"][0].sum(0)).all() and float(model.translation.grad[0, 2]) < 0  # descending moves the cube away


def test_kick_in_and_the_total(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*start(cuda, FRONT), *args, offset, human_faces=hf, occlusion=True)
    weights = with_do(kick_in=2, w=3.0)
    seen = []
    with torch.no_grad():
        for _ in range(3):
            total, terms = model(weights)
            seen.append(DO in terms)
    assert seen == [False, False, True] and model.step == 3
    rest = ((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0
    assert torch.equal(total, rest + terms[DO] * 3.0) and float(terms[DO]) > 0


def test_the_term_alone_moves_the_object_behind_the_body(hip_lib, cuda):
    """only the depth-order term, from the cube 0.3 in front of the body (fp64 Adam on the CPU: 1.110e-1 -> 5.69e-2 at iteration 10 ->
    an exact 0 from 32 on, Z from -0.6 to -0.34)"""
    args, offset, hf = scene(cuda)
    out = fit.fit_object_pose(*args, init=start(cuda, FRONT), hum_centroid_offset=offset, vars=("pose",), loss_weights=ONLY_DO, max_iter=40,
                              occlusion=True, human_faces=hf)
    history = out["history"][:, 0].tolist()
    z = float(out["translation"][0, 2])
    print(f"depth order, first -> last: {history[0]:.4e} -> {history[-1]:.4e}; translation Z {FRONT[2]} -> {z:.3f}")
    assert len(history) == 40 and history[0] > 5e-2
    assert history[-1] <= 0.5 * history[0]
    assert z > FRONT[2] + 0.1


def test_search_chunking_and_the_mirrored_start(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    weights = with_do()

    def run(chunk, centre, n=5):
        return fit.search_object_pose(*args, rotations=cube_rotations()[:n], init=(None, torch.tensor(centre, device=cuda), 1.0), icp=False,
                                      chunk=chunk, occlusion=True, human_faces=hf, hum_centroid_offset=offset, loss_weights=weights,
                                      max_iter=3)

    whole, parts = run(None, TRUE), run(2, TRUE)
    assert whole["rotation"].shape == (5, 6) and whole["history"].shape == (3, 5) and whole["scores"].shape == (5,)
    for k, v in whole.items():
        if isinstance(v, dict):
            assert all(torch.equal(v[j], parts[k][j]) for j in v), k
        else:
            assert torch.equal(v, parts[k]), k
    final = fit.ObjectPoseFit(whole["rotation"], whole["translation"], whole["scale"], *args, offset, fused_transform=True, human_faces=hf,
                              occlusion=True)
    with torch.no_grad():
        total, terms = final(weights, step=0)
    assert set(terms) == {"mask_loss", "centroid_loss", "contact_loss", DO}
    assert torch.equal(whole["scores"], total)
    assert torch.equal(total, (((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0) + terms[DO] * 10.0)
    # the same start mirrored to the wrong side of the body - in front of it, where the photo shows the body - ranks behind its twin
    wrong = run(None, MIRRORED, n=1)
    twin = fit.ObjectPoseFit(wrong["rotation"], wrong["translation"], wrong["scale"], *args, offset, fused_transform=True, human_faces=hf,
                             occlusion=True)
    with torch.no_grad():
        _, wrong_terms = twin(weights, step=0)
    print(f"scores: behind the body {float(whole['scores'][0]):.4f}, mirrored in front of it {float(wrong['scores'][0]):.4f}; depth order "
          f"{float(terms[DO][0]):.4e} against {float(wrong_terms[DO][0]):.4e}")
    assert float(wrong_terms[DO][0]) > float(terms[DO][0]) and float(wrong_terms[DO][0]) > 1e-2
    assert float(wrong["scores"][0]) > float(whole["scores"][0])


def test_refusals(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    with pytest.raises(ValueError, match="human_faces"):
        fit.ObjectPoseFit(*start(cuda), *args, offset, occlusion=True)
    with pytest.raises(ValueError, match="human_faces"):
        fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, occlusion=True, max_iter=2)
    model = fit.ObjectPoseFit(*start(cuda), *args, offset, human_faces=hf)
    with pytest.raises(ValueError, match="occlusion"):
        model(ONLY_DO)
    model(with_do(kick_in=-1))  # configured but off: nothing to refuse
    with pytest.raises(ValueError, match="occlusion"):
        fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, loss_weights=ONLY_DO, max_iter=2, human_faces=hf)
    # the device loop, by name
    for kwargs, name in ((dict(occlusion=True, human_faces=hf), "occlusion"), (dict(loss_weights=with_do()), DO),
                         (dict(loss_weights=with_do(), occlusion=True, human_faces=hf), DO)):
        with pytest.raises(ValueError, match=name):
            fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, max_iter=2, device_loop=True, **kwargs)
        with pytest.raises(ValueError, match=name):
            fit.search_object_pose(*args, rotations=cube_rotations()[:2], icp=False, device_loop=True, hum_centroid_offset=offset,
                                   max_iter=2, **kwargs)
    with pytest.raises(ValueError, match=DO):
        fit.DevicePoseFit(*start(cuda), *args, offset, loss_weights=with_do(), max_iter=2)
    with pytest.raises(ValueError, match="occlusion"):
        fit.DevicePoseFit(*start(cuda), *args, offset, max_iter=2, occlusion=True)
    prepared = fit.FitScene(*args, offset, human_faces=hf, occlusion=True)
    with pytest.raises(ValueError, match="occlusion"):  # a scene prepared with occlusion=True, which the loop would otherwise ignore
        fit.DevicePoseFit(*start(cuda), prepared, max_iter=2)
    # switched off, the device loop runs as before
    out = fit.fit_object_pose(*args, init=start(cuda), hum_centroid_offset=offset, loss_weights=with_do(kick_in=-1), max_iter=2,
                              device_loop=True)
    assert out["history"].shape == (2, 1)
