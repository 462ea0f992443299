"""interactvlm_amd.silhouette and interactvlm_amd.fit (csrc/silhouette.hip) on the GPU against tests/_silhouette_ref.py, the
documented definition in torch fp64 on the CPU (there is no pytorch3d golden).

Tolerances are derived from the documented error constants of the kernels (interactvlm_amd.silhouette.POS_ULPS, ...), not tuned:
    |alpha - alpha64| <= (1 - alpha) sum_k p_k |delta a_k| + (n_px + 4) 2^-24          (_silhouette_ref.alpha_bound)
    gradients: the same constants through the distance's derivative and the projection   (_silhouette_ref.grad_bound)
    silhouette_terms: (TERMS_CHAIN + 8) 2^-24 sum |terms|
The cut-off kappa d_k < blur_radius is a discontinuity: pixels where a face lies within the documented relative error of d of it
are left out of the comparison (gradient tests give them g_alpha = 0), and their share of the touched pixels is asserted <= 2 %.
"""
import functools
import math

import pytest
import torch

import _silhouette_ref as ref
from interactvlm_amd import contact_pair as cp
from interactvlm_amd import fit
from interactvlm_amd import silhouette as sil
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu

U = ref.U
CASES = [(*sc, bm) for sc in ref.SCENES for bm in (None, 3.0)]


@pytest.fixture(autouse=True)
def grad_enabled():
    """the whole suite reaches this file with autograd switched off for the process (see tests/test_contact_pair_gpu.py)"""
    with torch.enable_grad():
        yield


def assert_within(got, want, bound, what, mask=None):
    err = (got.detach().cpu().double() - want).abs()
    if mask is not None:
        err, bound = err[mask], bound[mask]
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst err / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"{what}: error exceeds the derived bound by {float((err - bound).max()):.3e}"


def gpu_alpha(cuda, verts, faces, cam, sigma, blur, grad=False):
    v = verts.to(cuda).requires_grad_(grad)
    a = sil.soft_silhouette(v, faces.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), sigma, blur)
    return v, a


@functools.lru_cache(maxsize=None)
def grad_case(*key):
    """the seeded g image (0 on the left-out pixels) and the fp64 autograd gradient of sum(g alpha), once per scene"""
    verts, faces, cam, blur, x = ref.case(*key)
    lo, _, _ = ref.left_out(x)
    g = torch.randn(cam.H, cam.W, generator=torch.Generator().manual_seed(7), dtype=torch.float64).float().double() * (~lo)
    with torch.enable_grad():
        v = verts.double().requires_grad_(True)
        (ref.render(v, faces, cam, x.sigma, blur) * g).sum().backward()
    return g, v.grad


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_alpha_against_fp64(hip_lib, cuda, key):
    verts, faces, cam, blur, x = ref.case(*key)
    lo, touched, guard = ref.left_out(x)
    share = float(lo.sum()) / float(touched.sum())
    bound = ref.alpha_bound(x)
    print(f"faces per pixel <= {int(x.counted.sum(1).max())}, guard {guard:.2e}, left out {int(lo.sum())} of {int(touched.sum())} "
          f"touched pixels, max bound {float(bound.max()):.2e}")
    assert share <= 0.02
    assert float(bound.max()) < 1e-3  # a face dropped at a tile or chunk edge shows far above this
    _, a = gpu_alpha(cuda, verts, faces, cam, key[4], blur)
    assert a.shape == (cam.H, cam.W) and a.dtype == torch.float32
    assert_within(a, x.alpha, bound, "alpha", ~lo)


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_vertex_gradient_against_fp64(hip_lib, cuda, key):
    verts, faces, cam, blur, x = ref.case(*key)
    g, want = grad_case(*key)
    v, a = gpu_alpha(cuda, verts, faces, cam, key[4], blur, grad=True)
    (a * g.float().to(cuda)).sum().backward()
    assert_within(v.grad, want, ref.grad_bound(x, g), "d sum(g alpha) / d verts")
    # depth moves the silhouette through u, v only, and it does move it
    assert float(want[:, 2].abs().max()) > 0 and float(v.grad[:, 2].abs().max()) > 0


def test_gradient_through_rot6d_and_translation(hip_lib, cuda):
    key = (12, 16, 33, 70, 4e-3, 3.0)
    verts, faces, cam, blur, x = ref.case(*key)
    g, gv64 = grad_case(*key)
    # the posed vertices are the identity transform of themselves: rot6d = first two columns of I, translation 0
    r6 = fit.matrix_to_rot6d(torch.eye(3))[0]
    J_r, J_t = torch.autograd.functional.jacobian(lambda r, t: fit.apply_transformation(verts.double(), r, t), (r6.double(), torch.zeros(3, dtype=torch.float64)))
    bound_v = ref.grad_bound(x, g)
    want_r, want_t = (J_r * gv64[..., None]).sum((0, 1)), (J_t * gv64[..., None]).sum((0, 1))
    rot, trans = torch.nn.Parameter(r6.to(cuda)), torch.nn.Parameter(torch.zeros(3, device=cuda))
    moved = fit.apply_transformation(verts.to(cuda), rot, trans)
    a = sil.soft_silhouette(moved, faces.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), key[4], blur)
    (a * g.float().to(cuda)).sum().backward()
    assert_within(rot.grad, want_r, (J_r.abs() * bound_v[..., None]).sum((0, 1)), "dL/drot6d")
    assert_within(trans.grad, want_t, (J_t.abs() * bound_v[..., None]).sum((0, 1)), "dL/dtranslation")
    assert float(trans.grad[2].abs()) > 0


def _unproject(uv, cam, z=3.0):
    uv = torch.tensor(uv, dtype=torch.float64)
    return torch.stack(((uv[:, 0] - cam.px) * z / cam.fx, (uv[:, 1] - cam.py) * z / cam.fy, torch.full((uv.shape[0],), z, dtype=torch.float64)), -1).float()


def test_triangle_larger_than_the_image(hip_lib, cuda):
    """one face, two vertices off-screen: its box is the whole image (5120 pixels: 80 steps of the one wave that walks it, more than
    one fp32 chain)"""
    cam = ref.camera(64, 80)
    verts = _unproject([(-60.0, -30.0), (150.0, 20.0), (30.0, 58.0)], cam)
    faces = torch.tensor([[0, 1, 2]])
    sigma = 4e-3
    for blur in (None, 3 * sigma):
        with torch.no_grad():
            x = ref.render(verts, faces, cam, sigma, blur, detail=True)
        lo, touched, _ = ref.left_out(x)
        assert float(lo.sum()) <= 0.02 * float(touched.sum())
        g = torch.randn(cam.H, cam.W, generator=torch.Generator().manual_seed(3), dtype=torch.float64).float().double() * (~lo)
        v64 = verts.double().requires_grad_(True)
        (ref.render(v64, faces, cam, sigma, blur) * g).sum().backward()
        v, a = gpu_alpha(cuda, verts, faces, cam, sigma, blur, grad=True)
        (a * g.float().to(cuda)).sum().backward()
        assert float(x.alpha.max()) > 0.999 and float(x.alpha.min()) < 1e-3
        assert_within(a, x.alpha, ref.alpha_bound(x), "alpha", ~lo)
        assert_within(v.grad, v64.grad, ref.grad_bound(x, g), "d sum(g alpha) / d verts")


def test_skipped_faces_change_nothing(hip_lib, cuda):
    """a face with a vertex at Z <= 0 and a face of zero area are skipped whole: the same bits as without them, gradient exactly 0"""
    key = (6, 8, 40, 48, 4e-3, 3.0)
    verts, faces, cam, blur, x = ref.case(*key)
    n = verts.shape[0]
    verts2 = torch.cat((verts, torch.tensor([[0.2, 0.1, -1.0], [0.0, 0.0, 0.0]])))
    faces2 = torch.cat((faces, torch.tensor([[3, 7, n], [5, n + 1, 9], [4, 4, 11], [2, 6, 6]])))
    g, _ = grad_case(*key)
    v, a = gpu_alpha(cuda, verts, faces, cam, key[4], blur, grad=True)
    (a * g.float().to(cuda)).sum().backward()
    v2, a2 = gpu_alpha(cuda, verts2, faces2, cam, key[4], blur, grad=True)
    (a2 * g.float().to(cuda)).sum().backward()
    assert torch.equal(a, a2)
    assert torch.equal(v.grad, v2.grad[:n])
    assert not bool(v2.grad[n:].any())
    with torch.no_grad():
        assert torch.equal(ref.render(verts2, faces2, cam, key[4], blur), x.alpha)  # the definition skips them too


def test_mesh_wholly_off_screen(hip_lib, cuda):
    verts, faces, cam, blur, _ = ref.case(6, 8, 40, 48, 4e-3, None)
    v = (verts + torch.tensor([100.0, 0.0, 0.0])).to(cuda).requires_grad_(True)
    a = sil.soft_silhouette(v, faces.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), 4e-3)
    target = torch.zeros(cam.H, cam.W, device=cuda)
    target[10:20, 12:30] = 1
    loss, centroid = sil.silhouette_terms(a, target)
    (loss + centroid.sum()).backward()
    assert not bool(a.any())
    assert centroid.tolist() == [cam.H / 2, cam.W / 2]
    assert float(loss.detach()) == 1.0
    assert not bool(v.grad.any()) and bool(torch.isfinite(v.grad).all())


def test_batch_determinism_and_graph_replay(hip_lib, cuda):
    key = (12, 16, 33, 70, 4e-3, 3.0)
    _, faces, cam, blur, _ = ref.case(*key)
    poses = torch.stack([ref.scene(12, 16, 33, 70, seed)[0] for seed in (0, 1, 2)]).to(cuda)
    f = faces.to(cuda)
    g = torch.randn(3, cam.H, cam.W, generator=torch.Generator().manual_seed(5)).to(cuda)

    def run(v):
        v = v.clone().requires_grad_(True)
        a = sil.soft_silhouette(v, f, (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), key[4], blur)
        a.backward(g[: a.shape[0]] if a.dim() == 3 else g[0])
        return a.detach(), v.grad

    a3, g3 = run(poses)
    assert a3.shape == (3, cam.H, cam.W)
    a3b, g3b = run(poses)
    assert torch.equal(a3, a3b) and torch.equal(g3, g3b)  # repeats are bit-equal
    for b in range(3):  # each pose of the batch is bit-equal to its own unbatched run
        ab = sil.soft_silhouette(poses[b], f, (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), key[4], blur)
        assert torch.equal(ab, a3[b])
        vb = poses[b].clone().requires_grad_(True)
        sil.soft_silhouette(vb, f, (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), key[4], blur).backward(g[b])
        assert torch.equal(vb.grad, g3[b])
    # graph capture and replay give the same bits (the topology cache is warm: capture makes no host read)
    static_v = poses.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            vg = static_v.clone().requires_grad_(True)
            ag = sil.soft_silhouette(vg, f, (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), key[4], blur)
            (gg,) = torch.autograd.grad(ag, vg, g)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ag, a3) and torch.equal(gg, g3)


def _terms_bound(alpha, target, gl, gc):
    """(TERMS_CHAIN + 8) 2^-24 sum |terms| for the loss, the centroid and the d / d alpha image, fp64"""
    C = (sil.TERMS_CHAIN + 8) * U
    H, W = alpha.shape
    a, t = alpha.double(), target.double()
    A, I, T = a.sum(), (a * t).sum(), t.sum()
    ii, jj = torch.arange(H, dtype=torch.float64)[:, None], torch.arange(W, dtype=torch.float64)[None]
    b_loss = C * (1 + (I / (A + T) if float(A + T) > 0 else 0.0))
    if float(A) > 0:
        c = torch.stack(((ii * a).sum(), (jj * a).sum())) / A
        b_c = C * c.abs()
        b_g = abs(gc[0]) * (ii + c[0]) / A + abs(gc[1]) * (jj + c[1]) / A
    else:
        b_c = C * torch.tensor([H / 2, W / 2])
        b_g = torch.zeros(H, W, dtype=torch.float64)
    if float(A + T) > 0:
        b_g = b_g + abs(gl) * (t * (A + T) + I) / (A + T) ** 2
    return b_loss, b_c, C * b_g


@pytest.mark.parametrize("name", ["random-33x70", "zero-33x70", "one-pixel-33x70", "random-1x1"])
def test_silhouette_terms_against_fp64(hip_lib, cuda, name):
    kind, shape = name.rsplit("-", 1)
    H, W = (int(v) for v in shape.split("x"))
    gen = torch.Generator().manual_seed(11)
    alpha = torch.rand(H, W, generator=gen)
    if kind == "zero":
        alpha.zero_()
    elif kind == "one-pixel":
        alpha.zero_()
        alpha[H // 3, W - 2] = 0.37
    target = (torch.rand(H, W, generator=gen) < 0.4).float()
    gl, gc = 0.7, (-1.3, 0.45)
    a64 = alpha.double().requires_grad_(True)
    loss64, c64 = ref.terms(a64, target)
    (gl * loss64 + gc[0] * c64[0] + gc[1] * c64[1]).backward()
    g64 = a64.grad if a64.grad is not None else torch.zeros(H, W, dtype=torch.float64)
    a = alpha.to(cuda).requires_grad_(True)
    loss, c = sil.silhouette_terms(a, target.to(cuda))
    assert loss.shape == () and c.shape == (2,)
    (gl * loss + gc[0] * c[0] + gc[1] * c[1]).backward()
    b_loss, b_c, b_g = _terms_bound(alpha, target, gl, gc)
    assert_within(loss, loss64.detach(), torch.as_tensor(b_loss), "mask_loss")
    assert_within(c, c64.detach(), b_c, "centroid")
    assert_within(a.grad, g64, b_g + 1e-300, "d / d alpha")
    if kind == "zero":
        assert c.tolist() == [H / 2, W / 2]
    # a batch with one shared target: every pose equals its own run, bit for bit
    ab = torch.stack((alpha, alpha.flip(0), alpha * 0.5)).to(cuda)
    lb, cb = sil.silhouette_terms(ab, target.to(cuda))
    assert lb.shape == (3,) and cb.shape == (3, 2)
    assert torch.equal(lb[0], loss.detach()) and torch.equal(cb[0], c.detach())


def test_memory_is_workspace_and_outputs(hip_lib, cuda):
    B, N, F, H, W = 1, 6890, 13776, 512, 512
    gen = torch.Generator().manual_seed(2)
    verts = (torch.randn(N, 3, generator=gen) * 0.3 + torch.tensor([0.0, 0.0, 3.0])).to(cuda)
    faces = torch.randint(N, (F, 3), generator=gen).to(cuda)
    args = ((900.0, 900.0), (256.0, 256.0), (H, W))
    sil.soft_silhouette(verts, faces, *args)  # builds the topology's incidence lists, which are kept
    v = verts.clone().requires_grad_(True)
    g = torch.ones(H, W, device=cuda)
    ws = hip_lib.ivlm_soft_silhouette_workspace_bytes(B, N, F, H, W)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sil.soft_silhouette(v, faces, *args).backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = ws + 4 * H * W + 12 * N + (1 << 20)
    print(f"peak memory rise {rise / 1e6:.2f} MB, workspace {ws / 1e6:.2f} MB, allowed {allowed / 1e6:.2f} MB "
          f"(a dense fp32 [H W, F] array: {H * W * F * 4 / 1e9:.1f} GB)")
    assert rise <= allowed
    assert bool(torch.isfinite(v.grad).all())


# ---- the fit ---------------------------------------------------------------------------------------------------------------------
def _rotation(axis, deg):
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    a = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


@functools.lru_cache(maxsize=None)
def fit_scene():
    """the 12 x 16 sphere at 64 x 64 against a human stand-in (an 8 x 12 sphere beside it), contact on the facing patches, the target
    mask rendered (fp64 definition) at a known pose, and two starts a few pixels and degrees off"""
    cam = ref.camera(64, 64)
    obj, faces = ref.uv_sphere(12, 16)
    hum, _ = ref.uv_sphere(8, 12)
    R_true = ref.random_rotation(1000)
    T_true = torch.tensor([0.1, -0.05, 3.0], dtype=torch.float64)
    posed = obj @ R_true + T_true
    hum = hum + torch.tensor([1.15, -0.05, 3.1], dtype=torch.float64)
    p_obj = ((posed[:, 0] - T_true[0]) > 0.3).float() * 0.8
    p_hum = ((hum[:, 0] - 1.15) < -0.3).float() * 0.6
    offset = torch.tensor([0.02, -0.01, 0.05])
    with torch.no_grad():
        target = ref.render((posed + offset.double()).float(), faces, cam, 1e-4) > 0.5
    starts = [(_rotation((1.0, 2.0, 0.5), 4.0), torch.tensor([0.10, -0.06, 0.08])), (_rotation((-1.0, 0.3, 1.0), -6.0), torch.tensor([-0.08, 0.09, -0.05]))]
    R6 = torch.cat([fit.matrix_to_rot6d((R_true @ dR).float()) for dR, _ in starts])
    T = torch.stack([T_true.float() + dT for _, dT in starts])
    return cam, obj.float(), faces, hum.float(), p_obj, p_hum, offset, target, R6, T


def _fit_step0_fp64(b, moved32):
    """total, terms and parameter gradients of start b at step 0 from the fp64 definitions, and their derived bounds.  moved32: the
    fp32 object vertices the kernels were given (the transform is plain torch, not the code under test), so that both sides
    evaluate the three terms at the same points; the parameter gradients are those vertex gradients through the fp64 Jacobian of
    the transform, with 16 u sum |J| |g| for the fp32 chain of the torch operations."""
    cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = fit_scene()
    H, W = cam.H, cam.W
    w = fit.DEFAULT_LOSS_WEIGHTS
    wm, wc, wk = w["mask_loss"]["w"], w["centroid_loss"]["w"], w["contact_loss"]["w"]
    moved = moved32.double().requires_grad_(True)
    offs = (moved32 + offset).double() - moved32.double()  # the offset as the fp32 addition applied it
    alpha = ref.render(moved + offs, faces, cam, 1e-4)
    alpha.retain_grad()
    mask_loss, centroid = ref.terms(alpha, target)
    c_target = fit.mask_bbox_centre(target.float()).double()
    centroid_loss = ((centroid - c_target) ** 2).sum()
    d = (moved[:, None, :] - hum.double()[None]).norm(dim=-1)
    pq = p_obj.double()[:, None] * p_hum.double()[None]
    contact = (pq * d).sum() / pq.sum()
    total = wm * mask_loss + wc * centroid_loss + wk * contact
    total.backward()
    with torch.no_grad():
        x = ref.render((moved + offs).detach(), faces, cam, 1e-4, detail=True)
        lo, _, _ = ref.left_out(x)
        ba = ref.alpha_bound(x)
        tt = target.double()
        A, I = x.alpha.sum(), (x.alpha * tt).sum()
        Um = A + tt.sum()
        ii = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
        jj = torch.arange(W, dtype=torch.float64)[None].expand(H, W)
        dA, dI = ba.sum(), (ba * tt).sum()  # what the alpha bound leaves of sum alpha and sum alpha t
        C = (sil.TERMS_CHAIN + 8) * U
        b_mask = (dI + I / Um * dA) / (Um - dA) + C * (1 + I / Um)
        c = centroid.detach()
        dc = torch.stack((((ii - c[0]).abs() * ba).sum(), ((jj - c[1]).abs() * ba).sum())) / (A - dA) + C * c.abs()
        b_centroid_loss = (2 * (c - c_target).abs() * dc + dc * dc).sum() + 4 * U * centroid_loss.detach()
        b_contact = (cp.L_CHAIN + 8) * U * contact.detach()
        # the error of g = d total / d alpha (through the sums), which the backward multiplies into every term
        g = alpha.grad.detach()
        dg = wm * ((tt * dA + dI) / Um ** 2 + 2 * (tt * Um - I).abs() * dA / Um ** 3) * 1.01
        second = wc * 2 * ((c[0] - c_target[0]) * (ii - c[0]) + (c[1] - c_target[1]) * (jj - c[1])) / A
        dg = dg + wc * 2 / A * (dc[0] * ((ii - c[0]).abs() + (c[0] - c_target[0]).abs()) + dc[1] * ((jj - c[1]).abs() + (c[1] - c_target[1]).abs())) * 1.01
        dg = dg + second.abs() * dA / A * 1.01 + 16 * U * g.abs()
        unit = (moved.detach()[:, None, :] - hum.double()[None]) / d.detach()[..., None]
        Ao = (pq[..., None] * unit.abs()).sum(1) / pq.sum()
        bound_v = ref.grad_bound(x, g) + ref.abs_terms(x, dg) + wk * (cp.L_CHAIN + 8) * U * Ao
    gv = moved.grad
    J_r, J_t = torch.autograd.functional.jacobian(lambda r, s: fit.apply_transformation(obj.double(), r, s), (R6[b].double(), T[b].double()))
    grads = []
    for J in (J_r, J_t):
        grads.append(((J * gv[..., None]).sum((0, 1)), (J.abs() * (bound_v + 16 * U * gv.abs())[..., None]).sum((0, 1))))
    terms = {"mask_loss": (mask_loss.detach(), b_mask), "centroid_loss": (centroid_loss.detach(), b_centroid_loss),
             "contact_loss": (contact.detach(), b_contact)}
    b_total = wm * b_mask + wc * b_centroid_loss + wk * b_contact + 4 * U * total.detach().abs()
    return (total.detach(), b_total), terms, grads[0], grads[1], lo


def _make_fit(cuda, sel):
    cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = fit_scene()
    return fit.ObjectPoseFit(R6[sel].to(cuda), T[sel].to(cuda), 1.0, obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda),
                             p_hum.to(cuda), target.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), offset.to(cuda))


def test_fit_step0_against_fp64(hip_lib, cuda):
    model = _make_fit(cuda, slice(0, 2))
    total, terms = model()
    total.sum().backward()
    assert total.shape == (2,) and set(terms) == {"mask_loss", "centroid_loss", "contact_loss"}
    moved = model.object_vertices().detach().cpu()
    for b in range(2):
        (t64, bt), terms64, (gr, br), (gt, btr), lo = _fit_step0_fp64(b, moved[b])
        # the mask and centroid terms sum over every pixel: a pixel at the cut-off cannot be left out of them, so there must be none
        assert int(lo.sum()) == 0, "choose another start: a face sits on the cut-off of the step-0 pose"
        for k, (v64, bk) in terms64.items():
            assert_within(terms[k][b], v64, torch.as_tensor(bk), f"start {b} {k}")
        assert_within(total[b], t64, torch.as_tensor(bt), f"start {b} total")
        assert_within(model.rotation.grad[b], gr, br, f"start {b} d total / d rot6d")
        assert_within(model.translation.grad[b], gt, btr, f"start {b} d total / d translation")


def test_fit_object_pose_descends_and_batches(hip_lib, cuda):
    cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = fit_scene()

    def run(sel):
        return fit.fit_object_pose(obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda),
                                   (cam.fx, cam.fy), (cam.px, cam.py), init=(R6[sel].to(cuda), T[sel].to(cuda), 1.0),
                                   hum_centroid_offset=offset.to(cuda), max_iter=30)

    both = run(slice(0, 2))
    hist = both["history"]
    assert hist.shape == (30, 2) and hist.is_cuda
    assert both["rotation"].shape == (2, 6) and both["translation"].shape == (2, 3) and both["object_vertices"].shape == (2, obj.shape[0], 3)
    print("total, first -> last:", hist[0].tolist(), "->", hist[-1].tolist())
    assert bool((hist[-1] < hist[0]).all())
    for b in range(2):  # B = 2 starts equal their own runs bit for bit
        own = run(slice(b, b + 1))
        assert torch.equal(own["history"][:, 0], hist[:, b])
        assert torch.equal(own["rotation"][0], both["rotation"][b]) and torch.equal(own["translation"][0], both["translation"][b])


def test_fit_object_pose_start_from_contact_icp(hip_lib, cuda):
    """init=None: the one start comes from contact_icp between the thresholded contact vertices of the two meshes"""
    cam, obj, faces, hum, p_obj, p_hum, offset, target, _, _ = fit_scene()
    out = fit.fit_object_pose(obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda),
                              (cam.fx, cam.fy), (cam.px, cam.py), hum_centroid_offset=offset.to(cuda), max_iter=30)
    hist = out["history"]
    assert hist.shape == (30, 1) and out["rotation"].shape == (1, 6) and out["translation"].shape == (1, 3) and out["scale"].shape == (1,)
    assert out["object_vertices"].shape == (1, obj.shape[0], 3)
    print("total, first -> last:", hist[0].tolist(), "->", hist[-1].tolist())
    assert bool(torch.isfinite(hist).all()) and bool((hist[-1] < hist[0]).all())
    # the rotation that comes back is still one
    R = fit.rot6d_to_matrix(out["rotation"])
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, device=cuda).expand(1, 3, 3), atol=1e-5)


def test_vertices_changed_before_backward_raise(hip_lib, cuda):
    verts, faces, cam, _, _ = ref.case(6, 8, 40, 48, 4e-3, None)
    v0 = verts.to(cuda).requires_grad_(True)
    v = v0 * 1.0
    a = sil.soft_silhouette(v, faces.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), 4e-3)
    v.add_(0.01)  # the boxes and 1 - alpha kept for the backward belong to the old coordinates
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        a.sum().backward()


def test_refusals(hip_lib, cuda):
    verts, faces, cam, _, _ = ref.case(6, 8, 40, 48, 4e-3, None)
    v, f = verts.to(cuda), faces.to(cuda)
    args = ((cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W))
    with pytest.raises(ValueError, match="float32"):
        sil.soft_silhouette(v.double(), f, *args)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        sil.soft_silhouette(v[:, :2], f, *args)
    with pytest.raises(ValueError, match="int32 or int64"):
        sil.soft_silhouette(v, f.float(), *args)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        sil.soft_silhouette(v, f[:, :2], *args)
    with pytest.raises(IvlmError, match="GPU tensor"):
        sil.soft_silhouette(verts, f, *args)
    with pytest.raises(IvlmError, match="GPU tensor"):
        sil.soft_silhouette(v, faces, *args)
    bad = f.clone()
    bad[3, 1] = v.shape[0]
    with pytest.raises(ValueError, match="vertex indices"):
        sil.soft_silhouette(v, bad, *args)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="vertex indices"):
        sil.soft_silhouette(v, bad, *args)
    for sigma in (0.0, -1e-4, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            sil.soft_silhouette(v, f, *args, sigma=sigma)
    with pytest.raises(ValueError, match="blur_radius"):
        sil.soft_silhouette(v, f, *args, blur_radius=-1.0)
    a = torch.rand(8, 9, device=cuda)
    with pytest.raises(ValueError, match="target_mask"):
        sil.silhouette_terms(a, torch.zeros(9, 8, device=cuda))
    with pytest.raises(ValueError, match="float32"):
        sil.silhouette_terms(a.double(), torch.zeros(8, 9, device=cuda))
    with pytest.raises(IvlmError, match="GPU tensor"):
        sil.silhouette_terms(a, torch.zeros(8, 9))
    # the C entry points refuse before any launch
    assert hip_lib.ivlm_soft_silhouette_workspace_bytes(1, 10, 10, 1 << 20, 16) == 0
    rc = hip_lib.ivlm_soft_silhouette_forward(v.data_ptr(), f.data_ptr(), 1, v.shape[0], f.shape[0], 40, 48, 72.0, 72.0, 24.0, 20.0,
                                              0.0, 1e-3, a.data_ptr(), a.data_ptr(), 1 << 30, None)
    assert rc == -4  # IVLM_ERR_UNSUPPORTED: sigma <= 0


def test_double_backward_raises(hip_lib, cuda):
    verts, faces, cam, _, _ = ref.case(6, 8, 40, 48, 4e-3, None)
    v = verts.to(cuda).requires_grad_(True)
    a = sil.soft_silhouette(v, faces.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), (cam.H, cam.W), 4e-3)
    # sum(alpha^2): the incoming gradient 2 alpha depends on the input, so a graph through the backward kernel would exist
    (gv,) = torch.autograd.grad((a * a).sum(), v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gv.sum().backward()
    al = torch.rand(8, 9, device=cuda, requires_grad=True)
    loss, _ = sil.silhouette_terms(al, torch.ones(8, 9, device=cuda))
    (ga,) = torch.autograd.grad(loss * loss, al, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        ga.sum().backward()
