"""``occlusion.depth_image`` and ``occlusion.depth_order`` (csrc/depth_order.hip) on the GPU against tests/_depth_order_ref.py.

The z-buffer is held to the reference's classification: at a DECIDED pixel the face index is the reference's and the depth lies within
the derived band; at an undecided one the answer is in the allowed set; undecided pixels are at most 2 % of the covered ones (the
reference alone gave 0 of 159 on the 24 x 40 scene and 3 of 509 on the 48 x 64 one).

The term's tolerance is ``K 2^-24 scale``, scale = the sum of the absolute per-pixel terms (for a gradient entry: of the absolute
per-pixel derivatives).  K is 4 x the largest error ratio of the SAME definition evaluated in torch fp32 on the CPU against fp64, over
exactly the inputs used here (``python tests/_depth_order_ref.py``; never taken from the kernel):

    case            L      gradient
    front           0.19   1584.35
    behind          0.78    635.12
    straddle       13.26    648.32
    straddle_soft  10.31    574.77
    pose            1.29     20.09      (through the reference's own Gram-Schmidt and transform in fp32)

    K_L = 4 x 13.26 -> 54,  K_G = 4 x 1584.35 -> 6338

The gradient's ratio is large because fp32 autograd takes d z / d e_i = 1 / t - s / (Z_i t^2) as a difference of nearly equal numbers on
a face that is nearly parallel to the image plane; the kernel takes the difference of the depths first.  The pose case is held to
the same K_L and K_G: the fused transform's own rounding has to fit inside them.
"""
import numpy as np
import pytest
import torch

import _depth_order_ref as ref
from interactvlm_amd import _lib, graphs, occlusion
from interactvlm_amd.pose import pose_transform

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_L, K_G = 54, 6338


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


_cases = {}


def order_case(name):
    """the reference's inputs and fp64 results, computed once and shared (never modified)"""
    if name not in _cases:
        _cases[name] = ref.pose_case() if name == "pose" else ref.order_case(name)
    return _cases[name]


def camera(cam):
    return (cam[0], cam[1]), (cam[2], cam[3])


def gpu_depth(v, f, cam, H, W, dev):
    d, k = occlusion.depth_image(torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev), *camera(cam), (H, W))
    assert d.shape == (1, H, W) and k.shape == (1, H, W) and d.dtype == torch.float32 and k.dtype == torch.int32
    return d[0].cpu().numpy(), k[0].cpu().numpy()


def hold_to_reference(depth, fid, cls):
    share = cls.undecided_share()
    dec = cls.decided
    with np.errstate(invalid="ignore"):  # (inf - inf on decided-empty pixels, which are not selected)
        err = np.abs(depth.astype(np.float64) - cls.depth)[dec & (cls.winner >= 0)]
    band = cls.band[dec & (cls.winner >= 0)]
    print(f"covered {int(cls.covered.sum())}, undecided {int((~dec).sum())} (share {share:.4f}); largest depth error / band "
          f"{(err / band).max() if err.size else 0.0:.3f}")
    assert share <= ref.UNDECIDED_CAP
    assert np.array_equal(fid[dec], cls.winner[dec])
    assert (err <= band).all()
    assert np.array_equal(np.isinf(depth) & (depth > 0), fid == -1)
    assert cls.contains(fid).all()


@pytest.mark.parametrize("which", ["small", "large"])
def test_depth_image_against_the_reference(hip_lib, cuda, which):
    """24 x 40 and 48 x 64: tile tails on both axes with 16 x 16 tiles, tiles the object never reaches; the large sphere has 1472
    faces (more than one 256-face chunk per tile) and faces smaller than a pixel"""
    v, f, cam, H, W = ref.scene(ref.SMALL if which == "small" else ref.LARGE)
    depth, fid = gpu_depth(v, f, cam, H, W, cuda)
    hold_to_reference(depth, fid, ref.classify(v, f, cam, H, W))
    assert (fid >= 0).sum() > 100 and (fid == -1).sum() > 100


def test_triangle_larger_than_the_image(hip_lib, cuda):
    _, _, cam, H, W = ref.scene(ref.SMALL)
    v = np.array([(-40.0, -30.0, 2.0), (50.0, -20.0, 3.0), (0.0, 60.0, 4.0)], dtype=np.float32)
    f = np.array([(0, 1, 2)], dtype=np.int64)
    cls = ref.classify(v, f, cam, H, W)
    assert cls.decided.all() and (cls.winner == 0).all()
    depth, fid = gpu_depth(v, f, cam, H, W, cuda)
    hold_to_reference(depth, fid, cls)
    assert depth.min() > 2.0 and depth.max() < 4.0


def test_skipped_faces_change_no_bit(hip_lib, cuda):
    v, f, cam, H, W = ref.scene(ref.SMALL)
    depth, fid = gpu_depth(v, f, cam, H, W, cuda)
    n = v.shape[0]
    extra_v = np.array([(0.0, 0.0, 1e-6), (0.1, 0.0, 0.0), (0.0, 0.1, -1.0)], dtype=np.float32)
    extra_f = np.array([(0, 1, n), (2, n + 1, 3), (n + 2, 4, 5),   # a vertex at Z = 1e-6, 0, -1
                        (7, 7, 9), (3, 8, 8)], dtype=np.int64)      # zero area: a repeated index
    depth2, fid2 = gpu_depth(np.concatenate([v, extra_v]), np.concatenate([f, extra_f]), cam, H, W, cuda)
    assert np.array_equal(depth.view(np.int32), depth2.view(np.int32)) and np.array_equal(fid, fid2)


def test_mesh_wholly_off_screen(hip_lib, cuda):
    v, f, cam, H, W = ref.scene(ref.SMALL)
    for shift in ((100.0, 0.0, 0.0), (0.0, -100.0, 0.0), (0.0, 0.0, -10.0)):  # beside, above, behind the camera
        depth, fid = gpu_depth(v + np.array(shift, dtype=np.float32), f, cam, H, W, cuda)
        assert (fid == -1).all() and np.isinf(depth).all() and (depth > 0).all()


def test_coincident_faces_the_lower_index_wins(hip_lib, cuda):
    v, f, cam, H, W = ref.scene(ref.SMALL)
    depth, fid = gpu_depth(v, f, cam, H, W, cuda)
    depth2, fid2 = gpu_depth(v, np.concatenate([f, f]), cam, H, W, cuda)  # every face a second time, at a higher index
    assert np.array_equal(depth.view(np.int32), depth2.view(np.int32)) and np.array_equal(fid, fid2) and fid2.max() < f.shape[0]


# ---- the term ---------------------------------------------------------------------------------------------------------------------
def run_order(k, dev, verts=None, B=None):
    f = torch.as_tensor(k["faces"]).to(dev)
    v = (torch.as_tensor(k["verts"]) if verts is None else verts).to(dev).clone().requires_grad_(True)
    occ, c = torch.as_tensor(k["occ"]).to(dev), torch.as_tensor(k["c"]).to(dev)
    L = occlusion.depth_order(v, f, occ, c, *camera(k["cam"]), k["tau"])
    return v, L


@pytest.mark.parametrize("name", list(ref.ORDER_CASES))
def test_depth_order_value_and_gradient_against_fp64(hip_lib, cuda, name):
    k = order_case(name)
    assert k["cls"].undecided_share() <= ref.UNDECIDED_CAP
    c = k["c"]
    assert (c > 0).any() and (c < 0).any() and (c == 0).any()
    v, L = run_order(k, cuda)
    assert L.shape == (1,)
    L.sum().backward()
    want = k["want"]
    got = float(L.detach()[0])
    rl, rg = ref.ratios(got, [v.grad.cpu().numpy()], want)
    print(f"{name}: L {got:.6e} (fp64 {want['L']:.6e}); ratios against fp64: L {rl:.2f} (<= {K_L}), gradient {rg:.2f} (<= {K_G})")
    assert want["A"] > 0 and np.abs(want["g"][0]).max() > 0
    assert rl <= K_L and rg <= K_G


def test_gradient_through_rot6d_and_translation(hip_lib, cuda):
    k = order_case("pose")
    assert k["cls"].undecided_share() <= ref.UNDECIDED_CAP
    base = torch.as_tensor(ref.uv_sphere(ref.SMALL[0], ref.SMALL[1])[0].astype(np.float32)).to(cuda)
    r6 = torch.as_tensor(k["r6"]).to(cuda).requires_grad_(True)
    t = torch.as_tensor(k["t"]).to(cuda).requires_grad_(True)
    v = pose_transform(base, r6[None], t[None], torch.ones(1, device=cuda))
    L = occlusion.depth_order(v, torch.as_tensor(k["faces"]).to(cuda), torch.as_tensor(k["occ"]).to(cuda),
                              torch.as_tensor(k["c"]).to(cuda), *camera(k["cam"]), k["tau"])
    L.sum().backward()
    want = k["want"]
    got = [r6.grad.cpu().numpy().astype(np.float64), t.grad.cpu().numpy().astype(np.float64)]
    rl, rg = ref.ratios(float(L.detach()[0]), got, want)
    print(f"pose: L {float(L.detach()[0]):.6e} (fp64 {want['L']:.6e}); ratios against fp64: L {rl:.2f} (<= {K_L}), gradient {rg:.2f} (<= {K_G})")
    assert want["A"] > 0 and all(np.abs(w).max() > 0 for w in want["g"])
    assert rl <= K_L and rg <= K_G


# ---- bit properties ---------------------------------------------------------------------------------------------------------------
def three_poses(k):
    v = torch.as_tensor(k["verts"])
    return torch.stack([v, v + torch.tensor([0.03, -0.02, 0.11]), v * torch.tensor([1.0, 0.9, 1.05])])


def test_batch_repeat_nan_workspace_and_graph_replay_give_the_same_bits(hip_lib, cuda):
    k = order_case("straddle_soft")
    H, W = k["H"], k["W"]
    poses = three_poses(k).to(cuda)
    f = torch.as_tensor(k["faces"]).to(cuda)
    occ, c = torch.as_tensor(k["occ"]).to(cuda), torch.as_tensor(k["c"]).to(cuda)
    gL = torch.tensor([0.7, -1.3, 2.0], device=cuda)
    focal, principal = camera(k["cam"])

    def run(v, g):
        v = v.clone().requires_grad_(True)
        L = occlusion.depth_order(v, f, occ, c, focal, principal, k["tau"])
        (gv,) = torch.autograd.grad(L, v, g)
        return L.detach(), gv

    L3, g3 = run(poses, gL)
    assert L3.shape == (3,) and g3.shape == poses.shape and bool((g3 != 0).any())
    L3b, g3b = run(poses, gL)
    assert torch.equal(L3, L3b) and torch.equal(g3, g3b)                     # two calls
    for b in range(3):                                                       # each pose of the batch against its own run
        Lb, gb = run(poses[b], gL[b:b + 1])
        assert torch.equal(Lb[0], L3[b]) and torch.equal(gb, g3[b])
    d3, k3 = occlusion.depth_image(poses, f, focal, principal, (H, W))
    for b in range(3):
        db, kb = occlusion.depth_image(poses[b], f, focal, principal, (H, W))
        assert torch.equal(db[0], d3[b]) and torch.equal(kb[0], k3[b])
    # the C calls on a workspace pre-filled with NaN bit patterns
    B, N, F = 3, poses.shape[1], f.shape[0]
    f32, offsets, slots = occlusion.silhouette.topology_of(f, N)
    nbytes = hip_lib.ivlm_depth_order_workspace_bytes(B, N, F, H, W)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=cuda)
    value = torch.full((B,), float("nan"), device=cuda)
    gv = torch.full((B, N, 3), float("nan"), device=cuda)
    cam = k["cam"]
    st = _lib.stream()
    assert hip_lib.ivlm_depth_order_forward(poses.data_ptr(), f32.data_ptr(), occ.data_ptr(), c.data_ptr(), B, N, F, H, W, *cam, k["tau"],
                                            value.data_ptr(), ws.data_ptr(), nbytes, st) == 0
    assert hip_lib.ivlm_depth_order_backward(poses.data_ptr(), offsets.data_ptr(), slots.data_ptr(), occ.data_ptr(), c.data_ptr(),
                                             gL.data_ptr(), B, N, F, H, W, *cam, k["tau"], gv.data_ptr(), ws.data_ptr(), nbytes, st) == 0
    assert torch.equal(value, L3) and torch.equal(gv, g3)
    nimg = hip_lib.ivlm_depth_image_workspace_bytes(B, N, F, H, W)
    ws = torch.full((nimg,), 0xFF, dtype=torch.uint8, device=cuda)
    d = torch.empty(B, H, W, device=cuda)
    ki = torch.empty(B, H, W, dtype=torch.int32, device=cuda)
    assert hip_lib.ivlm_depth_image(poses.data_ptr(), f32.data_ptr(), B, N, F, H, W, *cam, d.data_ptr(), ki.data_ptr(), ws.data_ptr(), nimg,
                                    st) == 0
    assert torch.equal(d, d3) and torch.equal(ki, k3)
    # graph capture and one replay of forward + backward (the topology cache is warm: the capture makes no host read)
    static = poses.clone()
    graph, (Lg, gg) = graphs.capture(lambda: run(static, gL), cuda)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Lg, L3) and torch.equal(gg, g3)


def test_double_backward_raises(hip_lib, cuda):
    k = order_case("straddle_soft")
    v, L = run_order(k, cuda)
    (gv,) = torch.autograd.grad((L * L).sum(), v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gv.sum().backward()


def test_no_weight_gives_an_exact_zero(hip_lib, cuda):
    k = dict(order_case("straddle"))
    k["c"] = np.zeros_like(k["c"])
    v, L = run_order(k, cuda)
    L.sum().backward()
    assert float(L.detach()[0]) == 0.0 and not bool(v.grad.any())


def test_memory_is_workspace_and_outputs(hip_lib, cuda):
    B, N, F, H, W = 1, 6890, 13776, 512, 512
    gen = torch.Generator().manual_seed(2)
    verts = (torch.randn(N, 3, generator=gen) * 0.3 + torch.tensor([0.0, 0.0, 3.0])).to(cuda)
    faces = torch.randint(N, (F, 3), generator=gen).to(cuda)
    occ = torch.full((H, W), 3.0, device=cuda)
    c = torch.ones(H, W, device=cuda)
    args = ((900.0, 900.0), (256.0, 256.0))
    occlusion.depth_order(verts, faces, occ, c, *args)  # builds the topology's incidence lists, which are kept
    v = verts.clone().requires_grad_(True)
    g = torch.ones(1, device=cuda)
    ws = hip_lib.ivlm_depth_order_workspace_bytes(B, N, F, H, W)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    occlusion.depth_order(v, faces, occ, c, *args).backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = ws + 4 * B + 12 * N + (1 << 20)
    print(f"peak memory rise {rise / 1e6:.2f} MB, workspace {ws / 1e6:.2f} MB, allowed {allowed / 1e6:.2f} MB "
          f"(a dense fp32 [H W, F] array: {H * W * F * 4 / 1e9:.1f} GB)")
    assert rise <= allowed
    assert bool(torch.isfinite(v.grad).all()) and bool((v.grad != 0).any())
