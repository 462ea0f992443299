"""The penetration term in the object-pose fit (fit.ObjectPoseFit / fit_object_pose / search_object_pose with human_faces).

The scene: the human is ``body_mesh(12, 11)`` at the origin, the object the 5 x 5 x 5 point cube of edge 0.2 with a 12-face box over
its corners, a 32 x 32 target mask, B <= 3.  The silhouette is rendered 3 units in front of the camera through hum_centroid_offset;
the contact and penetration terms live in the human's frame.  The starts (0, 0.4, 0.22) and (0.2, -0.5, 0.1) put part of the cube
inside the body, off its z = 0 symmetry plane, with unique closest points.  tol_g is the bound of tests/test_mesh_sdf_gpu.py:
K_G 2^-24 2 max d / N.
"""
import numpy as np
import pytest
import torch

import _mesh_sdf_ref as ref
from interactvlm_amd import fit
from interactvlm_amd import mesh_sdf as ms
from interactvlm_amd.pose import cube_rotations
from interactvlm_amd.synthetic import body_mesh
from test_mesh_sdf_gpu import K_G

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PEN = "penetration_loss"
ONLY_PEN = {PEN: {"w": 1.0, "kick_in": 0}}
CENTRES = ((0.0, 0.4, 0.22), (0.2, -0.5, 0.1))
IDENTITY6 = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)  # matrix_to_rot6d(eye): the first two columns, interleaved
FOCAL, PRINCIPAL = (48.0, 48.0), (17.3, 15.3)


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


def scene(dev):
    """-> (the eight positional scene arguments, offset, human_faces), on dev"""
    hum, hum_faces = body_mesh(12, 11)
    obj = torch.from_numpy(ref.point_cube()).float()
    corner = lambda c: (4 * (c >> 2 & 1)) * 25 + (4 * (c >> 1 & 1)) * 5 + 4 * (c & 1)  # noqa: E731  cube_mesh's corner -> grid index
    faces = torch.tensor([[corner(int(c)) for c in f] for f in ref.cube_mesh()[1]], dtype=torch.int32)
    p_obj = (obj[:, 1] < -0.04).float() * 0.8
    p_hum = (hum[:, 2] > 0.1).float() * 0.6
    target = torch.zeros(32, 32)
    target[13:19, 14:20] = 1.0
    offset = torch.tensor([0.0, 0.0, 3.0])
    args = tuple(t.to(dev) for t in (obj, faces, hum, p_obj, p_hum, target)) + (FOCAL, PRINCIPAL)
    return args, offset.to(dev), hum_faces.to(dev)


def starts(dev, sel=slice(None)):
    T = torch.tensor(CENTRES, device=dev)[sel]
    return torch.tensor(IDENTITY6, device=dev).repeat(T.shape[0], 1), T, 1.0


def with_pen(kick_in=0, w=3.0):
    return {**fit.DEFAULT_LOSS_WEIGHTS, PEN: {"w": w, "kick_in": kick_in}}


def test_identity_rot6d():
    assert torch.equal(fit.rot6d_to_matrix(torch.tensor(IDENTITY6))[0], torch.eye(3))


def test_term_alone(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*starts(cuda), *args, offset, human_faces=hf)
    total, terms = model(ONLY_PEN)
    assert set(terms) == {PEN} and total.shape == (2,)
    with torch.no_grad():
        moved = model.object_vertices()
        direct = ms.MeshSDF(args[2], hf).penetration(moved)
    assert torch.equal(total, terms[PEN]) and torch.equal(total, direct) and bool((total > 0).all())
    total.sum().backward()
    hum, faces = args[2].cpu().numpy(), hf.cpu().numpy()
    n = moved.shape[1]
    for b in range(2):
        x = moved[b].cpu().numpy()
        r = ref.query(x, hum, faces, unique=True)
        assert r["unique"].all() and 0 < r["inside"].sum() < n
        L64, g64, _ = ref.penetration(x, hum, faces, result=r)
        tol_g = K_G * U * 2.0 * r["d"][r["inside"]].max() / n
        err = np.abs(model.translation.grad[b].cpu().numpy().astype(np.float64) - g64.sum(0)).max()
        print(f"start {b}: L {float(total[b].detach()):.4e} (fp64 {L64:.4e}), |dL/dT - fp64| {err:.2e} <= {3 * tol_g * n:.2e}")
        assert err <= 3 * tol_g * n
    assert bool((model.rotation.grad != 0).any())


def test_default_weights_give_the_same_bits_with_and_without_faces(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    out = []
    for faces in (None, hf):
        model = fit.ObjectPoseFit(*starts(cuda), *args, offset, human_faces=faces)
        total, terms = model()
        total.sum().backward()
        out.append((total.detach(), terms, model.rotation.grad, model.translation.grad))
    (t0, terms0, gr0, gt0), (t1, terms1, gr1, gt1) = out
    assert set(terms0) == set(terms1) == {"mask_loss", "centroid_loss", "contact_loss"}
    assert torch.equal(t0, t1) and torch.equal(gr0, gr1) and torch.equal(gt0, gt1)
    assert all(torch.equal(terms0[k], terms1[k]) for k in terms0)
    # ... and with the key present but switched off
    model = fit.ObjectPoseFit(*starts(cuda), *args, offset, human_faces=hf)
    total, terms = model(with_pen(kick_in=-1))
    assert PEN not in terms and torch.equal(total, t0)


def test_kick_in(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    model = fit.ObjectPoseFit(*starts(cuda), *args, offset, human_faces=hf)
    weights = with_pen(kick_in=2)
    seen = []
    with torch.no_grad():
        for _ in range(3):
            total, terms = model(weights)
            seen.append(PEN in terms)
    assert seen == [False, False, True] and model.step == 3
    rest = ((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0
    assert torch.equal(total, rest + terms[PEN] * 3.0)


def test_term_on_without_faces_raises(hip_lib, cuda):
    args, offset, _ = scene(cuda)
    model = fit.ObjectPoseFit(*starts(cuda), *args, offset)
    with pytest.raises(ValueError, match="human_faces"):
        model(ONLY_PEN)
    model(with_pen(kick_in=-1))  # configured but off: nothing to refuse
    with pytest.raises(ValueError, match="human_faces"):
        fit.fit_object_pose(*args, init=starts(cuda), hum_centroid_offset=offset, loss_weights=ONLY_PEN, max_iter=2)


def test_device_loop_refuses_the_term(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    with pytest.raises(ValueError, match=PEN):
        fit.fit_object_pose(*args, init=starts(cuda), hum_centroid_offset=offset, loss_weights=with_pen(), max_iter=2, device_loop=True,
                            human_faces=hf)
    with pytest.raises(ValueError, match=PEN):
        fit.search_object_pose(*args, rotations=cube_rotations()[:2], icp=False, device_loop=True, human_faces=hf,
                               hum_centroid_offset=offset, loss_weights=with_pen(), max_iter=2)
    with pytest.raises(ValueError, match=PEN):  # and the class itself, which would otherwise leave the term out silently
        fit.DevicePoseFit(*starts(cuda), *args, offset, loss_weights=with_pen(), max_iter=2)
    # switched off, the device loop runs as before
    out = fit.fit_object_pose(*args, init=starts(cuda), hum_centroid_offset=offset, loss_weights=with_pen(kick_in=-1), max_iter=2,
                              device_loop=True, human_faces=hf)
    assert out["history"].shape == (2, 2)


def test_the_term_alone_pushes_the_object_out(hip_lib, cuda):
    """only the penetration term, rotation and translation free, 40 iterations from (0, 0.4, 0.22): the value at least halves.
    (A translation-only Adam at the project's learning rate reached an exact 0 by iteration 12 in fp64 on the CPU.)"""
    args, offset, hf = scene(cuda)
    out = fit.fit_object_pose(*args, init=starts(cuda, slice(0, 1)), hum_centroid_offset=offset, vars=("pose",), loss_weights=ONLY_PEN,
                              max_iter=40, human_faces=hf)
    history = out["history"][:, 0].tolist()
    print("penetration, first -> last:", history[0], "->", history[-1], "; first exact 0 at iteration",
          next((i for i, h in enumerate(history) if h == 0.0), None))
    assert history[0] > 0 and history[-1] < 0.5 * history[0]


def test_search_chunking_and_scores(hip_lib, cuda):
    args, offset, hf = scene(cuda)
    weights = with_pen()
    T0 = torch.tensor(CENTRES[0], device=cuda)

    def run(chunk):
        return fit.search_object_pose(*args, rotations=cube_rotations()[:6], init=(None, T0, 1.0), icp=False, chunk=chunk, human_faces=hf,
                                      hum_centroid_offset=offset, loss_weights=weights, max_iter=3)

    whole, parts = run(None), run(4)
    assert whole["rotation"].shape == (6, 6) and whole["history"].shape == (3, 6) and whole["scores"].shape == (6,)
    for k, v in whole.items():
        if isinstance(v, dict):
            assert all(torch.equal(v[j], parts[k][j]) for j in v), k
        else:
            assert torch.equal(v, parts[k]), k
    final = fit.ObjectPoseFit(whole["rotation"], whole["translation"], whole["scale"], *args, offset, fused_transform=True, human_faces=hf)
    with torch.no_grad():
        total, terms = final(weights, step=0)
    assert set(terms) == {"mask_loss", "centroid_loss", "contact_loss", PEN}
    assert torch.equal(whole["scores"], total)
    assert torch.equal(total, (((0.0 + terms["mask_loss"] * 5.0) + terms["centroid_loss"] * 1e-4) + terms["contact_loss"] * 10.0) + terms[PEN] * 3.0)
    assert bool((terms[PEN] > 0).any())  # the score really holds the term
