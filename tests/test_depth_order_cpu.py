"""The z-buffer and the depth-order term without a GPU: the yardstick of the GPU tests (tests/_depth_order_ref.py) against central
differences, its exact zero, its sign convention and its pixel classification; ``occluder_maps`` on hand-made images; every argument
refusal before the library loads; the C ABI's five new prototypes, its refusals before any launch, its workspace formula and version 5;
the fit's keys, signatures and refusals."""
import inspect

import numpy as np
import pytest
import torch

import _depth_order_ref as ref
from interactvlm_amd import _lib, fit, occlusion

DO = "depth_order_loss"


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


# ---- the reference against itself -------------------------------------------------------------------------------------------------
def test_reference_gradient_against_central_differences():
    k = ref.order_case("straddle_soft")
    v, f, cam, H, W = k["verts"], k["faces"], k["cam"], k["H"], k["W"]
    want = k["want"]
    assert want["A"] > 0 and np.abs(want["g"][0]).max() > 0
    _, fid0 = ref.depth_image(v, f, cam, H, W)
    h = 1e-7
    rows = np.argsort(-np.abs(want["g"][0]).max(1))[:6]  # the vertices with the largest gradients

    def value(vv):  # the winners found afresh: what central differences differentiate
        d, fid = ref.depth_image(vv, f, cam, H, W)
        assert np.array_equal(fid, fid0), "the step changed a winner or the covered set"
        win = np.where(k["cls"].decided, fid, -1)
        return float(ref.order_terms(torch.as_tensor(vv), f, win, cam, H, W, k["occ"], k["c"], k["tau"]).sum())

    base = v.astype(np.float64)
    worst = 0.0
    for n in rows:
        for ax in range(3):
            up, dn = base.copy(), base.copy()
            up[n, ax] += h
            dn[n, ax] -= h
            fd = (value(up) - value(dn)) / (2 * h)
            worst = max(worst, abs(fd - want["g"][0][n, ax]) / np.abs(want["g"][0]).max())
    print(f"central differences (h = {h}): largest error / largest gradient {worst:.2e}")
    assert worst < 1e-6


def test_reference_is_an_exact_zero_without_weights():
    k = ref.order_case("straddle")
    z = np.zeros_like(k["c"])
    out = ref.depth_order(k["verts"], k["faces"], k["winner"], k["cam"], k["H"], k["W"], k["occ"], z, k["tau"])
    assert out["L"] == 0.0 and out["A"] == 0.0 and not np.any(out["g"][0])


def quad(z, half=1.0):
    v = np.array([(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)], dtype=np.float32)
    return v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int64)


def test_sign_convention_on_two_fronto_parallel_quads():
    H = W = 8
    cam = (8.0, 8.0, 4.3, 3.8)
    (ov, of), (hv, hf) = quad(2.0), quad(3.0, half=4.0)
    d_o, fid = ref.depth_image(ov, of, cam, H, W)
    d_h, _ = ref.depth_image(hv, hf, cam, H, W)
    covered = np.isfinite(d_o)
    assert covered.sum() >= 30 and np.allclose(d_o[covered], 2.0, atol=1e-12) and np.isfinite(d_h).all() and np.allclose(d_h, 3.0, atol=1e-12)
    tau = 0.1

    def L(c):
        return ref.depth_order(ov, of, fid, cam, H, W, d_h, np.full((H, W), c, dtype=np.float32), tau)

    agree, clash = L(1.0), L(-1.0)  # the object IS in front: c > 0 agrees with the geometry, c < 0 contradicts it
    share = covered.sum() / (H * W)
    sp = lambda x: max(x, 0.0) + np.log1p(np.exp(-abs(x)))  # noqa: E731
    assert abs(agree["L"] - tau * share * sp(-10.0)) < 1e-15 and abs(clash["L"] - tau * share * sp(10.0)) < 1e-12
    assert clash["L"] > 1e4 * agree["L"]
    # descending the contradicted term moves the object away from the camera (behind the occluder), the agreeing one towards it
    assert clash["g"][0][:, 2].sum() < 0 and agree["g"][0][:, 2].sum() > 0
    # pixels the object does not cover add nothing but count in n; an occluder at +inf switches a pixel off
    gone = ref.depth_order(ov, of, fid, cam, H, W, np.full((H, W), np.inf), np.full((H, W), -1.0, dtype=np.float32), tau)
    assert gone["L"] == 0.0


def test_classification_of_the_two_scenes():
    """the undecided shares that the 2 % cap of the GPU tests is about, from the reference alone"""
    for which, at_most in ((ref.SMALL, 0.0), (ref.LARGE, ref.UNDECIDED_CAP)):
        v, f, cam, H, W = ref.scene(which)
        cls = ref.classify(v, f, cam, H, W)
        d, fid = ref.depth_image(v, f, cam, H, W)
        print(f"{which}: covered {int(cls.covered.sum())}, undecided {int((~cls.decided).sum())}")
        assert cls.undecided_share() <= at_most
        assert cls.contains(fid).all()                                   # fp64's own answer is always allowed
        assert np.array_equal(cls.winner[cls.decided], fid[cls.decided])
        assert np.array_equal(np.isfinite(d)[cls.decided], (cls.winner >= 0)[cls.decided])
        assert np.nanmax(cls.band) < 1e-3                                # the depth band is far below the front / back gap (> 1e-2)


# ---- occluder_maps ----------------------------------------------------------------------------------------------------------------
def test_occluder_maps_on_hand_made_images(monkeypatch):
    inf = float("inf")
    d_h = torch.tensor([[1.0, 2.0, inf], [inf, 3.0, 4.0]])
    target = torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 7.0]])
    d, sw, valid = occlusion.maps_from_depth(d_h, target)
    assert d is d_h
    assert torch.equal(sw, torch.tensor([[1.0, -1.0, 0.0], [0.0, -1.0, 1.0]]))
    assert torch.equal(valid, torch.tensor([[1.0, 0.0, 1.0], [1.0, 0.0, 1.0]]))
    assert torch.equal((target != 0).float() * valid, (target != 0).float())
    # the photo's person mask replaces the rendered cover
    mask = torch.tensor([[0, 1, 1], [1, 0, 1]], dtype=torch.uint8)
    _, sw, valid = occlusion.maps_from_depth(d_h, target, mask)
    assert torch.equal(sw, torch.tensor([[0.0, -1.0, 1.0], [-1.0, 0.0, 1.0]]))
    assert torch.equal(valid, torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]))
    # occluder_maps itself: the human's depth image, then that arithmetic
    monkeypatch.setattr(_lib, "require_gpu", lambda named: None)
    seen = []

    def fake_depth(verts, faces, focal, principal, image_size):
        seen.append((tuple(verts.shape), image_size))
        return d_h[None], torch.zeros(1, 2, 3, dtype=torch.int32)

    monkeypatch.setattr(occlusion, "depth_image", fake_depth)
    hv, hf = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    d, sw, valid = occlusion.occluder_maps(hv, hf, target, 10.0, (1.5, 1.0))
    assert seen == [((4, 3), (2, 3))] and torch.equal(d, d_h) and torch.equal(sw, torch.tensor([[1.0, -1.0, 0.0], [0.0, -1.0, 1.0]]))


# ---- refusals before the library loads --------------------------------------------------------------------------------------------
def test_every_argument_refusal_comes_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    v, f = torch.zeros(5, 3), torch.tensor([[0, 1, 2]])
    img = torch.zeros(4, 6)
    cam = (10.0, (3.0, 2.0))
    for bad, name in ((dict(verts=torch.zeros(5, 2)), "verts"), (dict(verts=v.double()), "verts"), (dict(verts="x"), "verts"),
                      (dict(faces=torch.zeros(1, 4, dtype=torch.int64)), "faces"), (dict(faces=f.float()), "faces"),
                      (dict(focal="f"), "focal"), (dict(principal=(1.0, float("nan"))), "principal"), (dict(image_size=(0, 4)), "image_size")):
        args = dict(verts=v, faces=f, focal=cam[0], principal=cam[1], image_size=(4, 6))
        args.update(bad)
        with pytest.raises(ValueError, match=name):
            occlusion.depth_image(**args)
    with pytest.raises(_lib.IvlmError, match="GPU"):
        occlusion.depth_image(v, f, *cam, (4, 6))
    for bad, name in ((dict(occluder_depth=torch.zeros(4)), "occluder_depth"), (dict(occluder_depth=img.double()), "occluder_depth"),
                      (dict(signed_weight=torch.zeros(4, 5)), "signed_weight"), (dict(signed_weight=img.bool()), "signed_weight"),
                      (dict(signed_weight=None), "signed_weight"), (dict(tau=0.0), "tau"), (dict(tau=float("inf")), "tau"),
                      (dict(tau="t"), "tau"), (dict(verts=torch.zeros(2, 5, 4)), "verts"), (dict(faces=None), "faces")):
        args = dict(verts=v, faces=f, occluder_depth=img, signed_weight=img, focal=cam[0], principal=cam[1], tau=0.01)
        args.update(bad)
        with pytest.raises(ValueError, match=name):
            occlusion.depth_order(**args)
    with pytest.raises(_lib.IvlmError, match="GPU"):
        occlusion.depth_order(v, f, img, img, *cam)
    with pytest.raises(ValueError, match="target_mask"):
        occlusion.occluder_maps(v, f, torch.zeros(4), *cam)
    with pytest.raises(ValueError, match="human_verts"):
        occlusion.occluder_maps(torch.zeros(2, 5, 3), f, img, *cam)
    with pytest.raises(ValueError, match="human_mask"):
        occlusion.occluder_maps(v, f, img, *cam, human_mask=torch.zeros(4, 5))
    with pytest.raises(_lib.IvlmError, match="GPU"):
        occlusion.occluder_maps(v, f, img, *cam)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def names(args):
    return [a.split()[-1].lstrip("*") for a in args]


def test_header_declares_the_five_entry_points_and_the_abi_is_still_5():
    protos = _lib.header_prototypes()
    sizes = ["int B", "int N", "int F", "int H", "int W"]
    assert protos["ivlm_depth_image_workspace_bytes"] == ("size_t", sizes)
    assert protos["ivlm_depth_order_workspace_bytes"] == ("size_t", sizes)
    cam = ["B", "N", "F", "H", "W", "fx", "fy", "px", "py"]
    tail = ["workspace", "workspace_bytes", "stream"]
    assert names(protos["ivlm_depth_image"][1]) == ["verts", "faces"] + cam + ["depth_out", "face_id_out"] + tail
    assert names(protos["ivlm_depth_order_forward"][1]) == ["verts", "faces", "occluder_depth", "signed_weight"] + cam + ["tau", "value_out"] + tail
    assert names(protos["ivlm_depth_order_backward"][1]) == (["verts", "vert_face_offsets", "vert_face_list", "occluder_depth", "signed_weight",
                                                              "grad_value"] + cam + ["tau", "grad_verts_out"] + tail)
    assert all(protos[n][0] == "int" for n in ("ivlm_depth_image", "ivlm_depth_order_forward", "ivlm_depth_order_backward"))
    text = open(_lib.HEADER_PATH).read()
    assert "IvlmFitStepArgs" in text and _lib.header_constant("IVLM_DEPTH_ORDER_CHAIN") == occlusion.L_CHAIN == 32
    assert _lib.load().ivlm_abi_version() == 5


def test_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake, big = 4096, 1 << 40  # pointers that are never followed: the refusals below come before any launch
    cam = [10.0, 10.0, 3.0, 2.0]
    calls = ((lib.ivlm_depth_image, [fake, fake, 1, 5, 4, 8, 8, *cam, fake, fake, fake, big, None], (0, 1, 11, 12, 13), None),
             (lib.ivlm_depth_order_forward, [fake, fake, fake, fake, 1, 5, 4, 8, 8, *cam, 0.01, fake, fake, big, None], (0, 1, 2, 3, 14, 15), 13),
             (lib.ivlm_depth_order_backward, [fake, fake, fake, fake, fake, fake, 1, 5, 4, 8, 8, *cam, 0.01, fake, fake, big, None],
              (0, 1, 2, 3, 4, 5, 16, 17), 15))
    for call, ok, pointers, tau_at in calls:
        first = next(i for i, a in enumerate(ok) if a == 1)  # B
        ws = len(ok) - 3
        for at in pointers:
            bad = list(ok)
            bad[at] = None
            assert call(*bad) == -1, (call.__name__, at)
        for at, v in ((first, 0), (first, 65536), (first + 1, 0), (first + 1, (1 << 22) + 1), (first + 2, (1 << 22) + 1), (first + 3, 16385),
                      (first + 4, -1), (first + 5, float("nan")), (first + 8, float("inf"))):
            bad = list(ok)
            bad[at] = v
            assert call(*bad) == -4, (call.__name__, at, v)
        if tau_at is not None:
            for v in (0.0, -1.0, float("nan"), float("inf")):
                bad = list(ok)
                bad[tau_at] = v
                assert call(*bad) == -4, (call.__name__, v)
        query = lib.ivlm_depth_image_workspace_bytes if tau_at is None else lib.ivlm_depth_order_workspace_bytes
        bad = list(ok)
        bad[ws + 1] = query(1, 5, 4, 8, 8) - 1
        assert call(*bad) == -2
        bad = list(ok)
        bad[ws] = fake + 4  # a workspace off its alignment
        assert call(*bad) == -2


def test_workspace_formulas():
    lib = _lib.load()
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    for B, N, F, H, W in ((1, 1, 1, 1, 1), (3, 42, 80, 24, 40), (1, 6890, 13776, 512, 512), (24, 738, 1472, 48, 64)):
        image = pad(8 * B * N) + pad(48 * B * F) + pad(16 * B * F) + pad(16 * B)
        assert lib.ivlm_depth_image_workspace_bytes(B, N, F, H, W) == image
        assert lib.ivlm_depth_order_workspace_bytes(B, N, F, H, W) == (image + 2 * pad(4 * B * H * W) + pad(36 * B * F) + pad(16 * B * H)
                                                                      + pad(16 * B))
    for bad in ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 16385), (65536, 4, 4, 8, 8),
                (1, (1 << 22) + 1, 4, 8, 8)):
        assert lib.ivlm_depth_image_workspace_bytes(*bad) == 0 and lib.ivlm_depth_order_workspace_bytes(*bad) == 0


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def test_fit_keys_and_signatures():
    assert fit.TERM_KEYS == ("mask_loss", "centroid_loss", "contact_loss")
    assert fit.TERMS[DO] is None and fit.DEPTH_ORDER_KEY == DO and DO not in fit.DEFAULT_LOSS_WEIGHTS
    assert (fit.PENETRATION_KEY, fit.INTRUSION_KEY) == ("penetration_loss", "intrusion_loss")
    for fn in (fit.FitScene.__init__, fit.ObjectPoseFit.__init__, fit.fit_object_pose, fit.search_object_pose):
        p = inspect.signature(fn).parameters
        assert p["occlusion"].default is False and p["human_mask"].default is None and p["depth_tau"].default == 0.01
    assert fit.FitScene._DEFAULTS == (None,) * 8 + (1e-4, None, False, None, False, None, 0.01)
    assert len(fit.FitScene._DEFAULTS) == len(inspect.signature(fit.FitScene.__init__).parameters) - 2
    assert "tau" in occlusion.depth_order.__doc__ and "nobody has measured" in occlusion.depth_order.__doc__


def test_fit_refusals_raise_before_the_library_loads(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    weights = {DO: {"w": 1.0, "kick_in": 0}}
    with pytest.raises(ValueError, match=DO):
        fit.fit_object_pose(*[None] * 8, init=(None, None, 1.0), loss_weights=weights, device_loop=True)
    with pytest.raises(ValueError, match=DO):
        fit.search_object_pose(*[None] * 8, loss_weights=weights, device_loop=True)
    with pytest.raises(ValueError, match=DO):
        fit.DevicePoseFit(*[None] * 11, loss_weights=weights)
    with pytest.raises(ValueError, match="occlusion"):
        fit.fit_object_pose(*[None] * 8, init=(None, None, 1.0), device_loop=True, occlusion=True)
    with pytest.raises(ValueError, match="occlusion"):
        fit.search_object_pose(*[None] * 8, device_loop=True, occlusion=True)
    with pytest.raises(ValueError, match="occlusion"):
        fit.DevicePoseFit(*[None] * 11, occlusion=True)
    # occlusion=True without the human's triangles is refused by name, before anything is prepared
    args = (torch.tensor([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]), torch.zeros(1, 3), 1.0, torch.zeros(8, 3), torch.zeros(12, 3, dtype=torch.int64),
            torch.zeros(4, 3), torch.zeros(8), torch.zeros(4), torch.zeros(8, 8), (10.0, 10.0), (4.0, 4.0))
    with pytest.raises(ValueError, match="human_faces"):
        fit.ObjectPoseFit(*args, occlusion=True)
    with pytest.raises(ValueError, match="tau"):
        fit.ObjectPoseFit(*args, depth_tau=0.0)
    # human_faces stays the last parameter: passed by position behind intrusion it lands in occlusion, which says so by name
    faces = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="occlusion.*human_faces"):
        fit.ObjectPoseFit(*args, None, ("pose",), 1e-4, None, False, False, faces)
    with pytest.raises(ValueError, match="occlusion.*human_faces"):
        fit.fit_object_pose(*args[3:], None, None, ("pose",), None, 2, False, 1e-4, None, (0.3, 0.5), 10, True, True, False, faces)
    # the occlusion images are buffers of the model (None without occlusion=True, and then in no state_dict)
    model = fit.ObjectPoseFit(*args)
    assert model.valid is None and model.occluder_depth is None and model.signed_weight is None
    assert not {"valid", "occluder_depth", "signed_weight"} & set(model.state_dict())
    # the term on, on a model built without occlusion=True (CPU tensors: the refusal comes before any kernel)
    model = fit.ObjectPoseFit(*args)
    with pytest.raises(ValueError, match="occlusion"):
        model(weights)
