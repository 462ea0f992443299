"""interactvlm_amd.pose (csrc/pose.hip) and the multi-start search of interactvlm_amd.fit on the GPU.

The yardsticks are the project's own fp64 definitions on the CPU: autograd through fit.apply_transformation on fp64 copies, the
fp64 restatement of the fit step in tests/test_silhouette_gpu.py, and the fp64 search of tests/_pose_scene.py (its 24 finals are
the fixture tests/golden/pose_search_fp64.json).  Bounds come from the documented constants of the kernels (pose.FWD_ULPS,
pose.GRAD_ULPS), never from a measurement:
    forward     FWD_ULPS 2^-24 (s sum_i |v_i| |R_ij| + |t_j|) per coordinate
    gradients   GRAD_ULPS 2^-24 sum_n |J_n| |g_n| with the fp64 absolute Jacobian of the transform
"""
import functools

import pytest
import torch

import _pose_scene as ps
import _silhouette_ref as ref
import test_silhouette_gpu as tsg
from interactvlm_amd import fit, pose
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu

U = ref.U
CH = pose.POSE_CHUNK
assert_within = tsg.assert_within


@pytest.fixture(autouse=True)
def grad_enabled():
    """the whole suite reaches this file with autograd switched off for the process (see tests/test_contact_pair_gpu.py)"""
    with torch.enable_grad():
        yield


def make_inputs(N, B, seed, tensor_scale):
    """seeded vertices of magnitude ~1, a NON-orthonormal rot6d (a rotation's columns scaled by 0.7 and 1.9, plus noise), t of
    magnitude ~3, s a [B] tensor around 0.8 - 1.3 or the number 1.0, an upstream g of normals"""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(N, 3, generator=gen)
    r6 = []
    for b in range(B):
        R = ref.random_rotation(100 * seed + b)
        a1 = 0.7 * R[:, 0] + 0.05 * torch.randn(3, generator=gen, dtype=torch.float64)
        a2 = 1.9 * R[:, 1] + 0.05 * torch.randn(3, generator=gen, dtype=torch.float64)
        r6.append(torch.stack((a1, a2), -1).reshape(6).float())
    r6 = torch.stack(r6)
    t = 3.0 * torch.randn(B, 3, generator=gen)
    s = (0.8 + 0.5 * torch.rand(B, generator=gen)) if tensor_scale else 1.0
    g = torch.randn(B, N, 3, generator=gen)
    return v, r6, t, s, g


def reference(v, r6, t, s, g):
    """fp64 on the CPU: the output, the gradients of sum(g out) by autograd through fit.apply_transformation, and the derived
    bounds.  The transform is linear in R, so its absolute Jacobian is exact from d R / d rot6d (autograd, 9 x 6 per pose):
    d y_nj / d r_k = s sum_i v_ni dR_ij/dr_k,  d y_nj / d t_j = 1,  d y_nj / d s = (v_n R)_j."""
    B = r6.shape[0]
    v64, g64 = v.double(), g.double()
    r64, t64 = r6.double().requires_grad_(True), t.double().requires_grad_(True)
    tensor_scale = isinstance(s, torch.Tensor)
    s64 = s.double().requires_grad_(True) if tensor_scale else torch.full((B,), float(s), dtype=torch.float64)
    with torch.enable_grad():
        out = fit.apply_transformation(v64, r64, t64, s64)
        (out * g64).sum().backward()
    with torch.no_grad():
        R = fit.rot6d_to_matrix(r64)
        sv = s64.detach()[:, None, None] * v64.abs()[None]
        b_out = pose.FWD_ULPS * U * (torch.einsum("bni,bij->bnj", sv, R.abs()) + t64.detach().abs()[:, None, :])
    D = torch.stack([torch.autograd.functional.jacobian(lambda r: fit.rot6d_to_matrix(r)[0], r64[b].detach()) for b in range(B)])  # [B,3,3,6]
    with torch.no_grad():
        J_r = torch.einsum("b,ni,bijk->bnjk", s64.detach(), v64, D)
        C = pose.GRAD_ULPS * U
        b_r = C * (J_r.abs() * g64.abs()[..., None]).sum((1, 2))
        b_t = C * g64.abs().sum(1)
        b_s = C * (torch.einsum("ni,bij->bnj", v64, R).abs() * g64.abs()).sum((1, 2))
    return out.detach(), (r64.grad, t64.grad, s64.grad if tensor_scale else None), b_out, (b_r, b_t, b_s)


def run_gpu(cuda, v, r6, t, s, g, grads=(True, True, True)):
    r = r6.to(cuda).requires_grad_(grads[0])
    tt = t.to(cuda).requires_grad_(grads[1])
    ss = s.to(cuda).requires_grad_(grads[2]) if isinstance(s, torch.Tensor) else s
    out = pose.pose_transform(v.to(cuda), r, tt, ss)
    if out.requires_grad:
        out.backward(g.to(cuda))
    return out.detach(), (r.grad, tt.grad, ss.grad if isinstance(s, torch.Tensor) else None)


def check_against_fp64(cuda, v, r6, t, s, g, what):
    out64, grads64, b_out, bounds = reference(v, r6, t, s, g)
    out, grads = run_gpu(cuda, v, r6, t, s, g)
    assert out.shape == out64.shape and out.dtype == torch.float32
    assert_within(out, out64, b_out, f"{what} forward")
    for got, want, bound, name in zip(grads, grads64, bounds, ("rot6d", "translation", "scale")):
        if want is None:
            assert got is None
            continue
        assert float(want.abs().max()) > 0
        assert_within(got, want, bound + 1e-300, f"{what} dL/d{name}")


@pytest.mark.parametrize("tensor_scale", [False, True], ids=["s=1.0", "s=tensor"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, CH, CH + 1, 2 * CH + 5])
def test_forward_and_gradients_against_fp64(hip_lib, cuda, N, B, tensor_scale):
    v, r6, t, s, g = make_inputs(N, B, seed=N % 97 + B, tensor_scale=tensor_scale)
    check_against_fp64(cuda, v, r6, t, s, g, f"N={N} B={B}")
    if B == 1:  # the unbatched form: [6], [3] and a 0-dim scale give [N,3] with the bits of the B = 1 batch
        s0 = s[0] if tensor_scale else s
        one = pose.pose_transform(v.to(cuda), r6[0].to(cuda), t[0].to(cuda), s0.to(cuda) if tensor_scale else s0)
        assert one.shape == (N, 3)
        assert torch.equal(one, run_gpu(cuda, v, r6, t, s, g)[0][0])


@pytest.mark.parametrize("vertex", [2 * CH + 4, CH - 1, CH], ids=["last", "chunk-end", "chunk-start"])
def test_tail_and_chunk_edges(hip_lib, cuda, vertex):
    """g zero except at ONE vertex - the last of the tail chunk, the last of a full chunk, the first of the next: dL/dt is that row
    bit for bit, the other gradients are the single-vertex closed form"""
    N, B = 2 * CH + 5, 2
    v, r6, t, s, g = make_inputs(N, B, seed=3, tensor_scale=True)
    row = g[:, vertex].clone()
    g.zero_()
    g[:, vertex] = row
    _, (g_r, g_t, g_s) = run_gpu(cuda, v, r6, t, s, g)
    assert torch.equal(g_t.cpu(), row)
    _, (w_r, _, w_s), _, (b_r, _, b_s) = reference(v[vertex:vertex + 1], r6, t, s, row[:, None, :])
    assert_within(g_r, w_r, b_r, f"vertex {vertex} dL/drot6d")
    assert_within(g_s, w_s, b_s, f"vertex {vertex} dL/dscale")
    assert float(w_r.abs().min()) > 0 and float(w_s.abs().min()) > 0


def test_zero_upstream_gives_zero_gradients(hip_lib, cuda):
    v, r6, t, s, g = make_inputs(2 * CH + 5, 2, seed=4, tensor_scale=True)
    _, grads = run_gpu(cuda, v, r6, t, s, torch.zeros_like(g))
    for got in grads:
        assert not bool(got.any()) and bool(torch.isfinite(got).all())


def test_batch_determinism_and_graph_replay(hip_lib, cuda):
    N = 2 * CH + 5
    v, r6, t, s, g = make_inputs(N, 3, seed=5, tensor_scale=True)
    alone = run_gpu(cuda, v, r6[:1], t[:1], s[:1], g[:1])
    again = run_gpu(cuda, v, r6[:1], t[:1], s[:1], g[:1])
    assert torch.equal(alone[0], again[0]) and all(torch.equal(a, b) for a, b in zip(alone[1], again[1]))  # repeats are bit-equal
    for place in range(3):  # the same pose (and its upstream gradient) as member 0, 1 and 2 of a batch of three
        order = [(k - place) % 3 for k in range(3)]  # batch[place] is pose 0
        out, grads = run_gpu(cuda, v, r6[order], t[order], s[order], g[order])
        assert torch.equal(out[place], alone[0][0]), f"forward bits differ as member {place}"
        for got, want, name in zip(grads, alone[1], ("rot6d", "translation", "scale")):
            assert torch.equal(got[place], want[0]), f"dL/d{name} bits differ as member {place}"
    # graph capture and two replays give the bits of the eager call
    want_out, want_grads = run_gpu(cuda, v, r6, t, s, g)
    vc, gc = v.to(cuda), g.to(cuda)
    static = [x.to(cuda) for x in (r6, t, s)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            leaves = [x.clone().requires_grad_(True) for x in static]
            out = pose.pose_transform(vc, *leaves)
            got_grads = torch.autograd.grad(out, leaves, gc)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), want_out)
        assert all(torch.equal(a, b) for a, b in zip(got_grads, want_grads))


def _search_model(cuda, vars, B=2):
    cam, obj, faces, hum, p_obj, p_hum, target, T_start = ps.search_scene()
    r6, T, s = pose.pose_starts(pose.cube_rotations()[6:6 + B].to(cuda), None, T_start.to(cuda), 1.0)
    return fit.ObjectPoseFit(r6, T, s, obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda),
                             (cam.fx, cam.fy), (cam.px, cam.py), vars=vars, fused_transform=True)


def test_which_gradients_are_produced(hip_lib, cuda):
    model = _search_model(cuda, ("pose",))
    model()[0].sum().backward()
    assert model.rotation.grad is not None and model.translation.grad is not None
    assert not model.scale.requires_grad and model.scale.grad is None
    model = _search_model(cuda, ("scale",))
    model()[0].sum().backward()
    assert model.rotation.grad is None and model.translation.grad is None
    assert model.scale.grad.shape == (2,) and bool(torch.isfinite(model.scale.grad).all()) and bool((model.scale.grad != 0).all())
    model = _search_model(cuda, ("pose", "scale"))
    model()[0].sum().backward()
    assert all(p.grad is not None for p in (model.rotation, model.translation, model.scale))
    # the function itself: an input that does not require grad gets none, and the others do not change a bit for it
    v, r6, t, s, g = make_inputs(CH + 1, 2, seed=6, tensor_scale=True)
    full = run_gpu(cuda, v, r6, t, s, g)[1]
    for keep in range(3):
        grads = run_gpu(cuda, v, r6, t, s, g, grads=tuple(k == keep for k in range(3)))[1]
        assert [x is not None for x in grads] == [k == keep for k in range(3)]
        assert torch.equal(grads[keep], full[keep])


def test_fused_step0_against_fp64(hip_lib, cuda):
    """ObjectPoseFit(fused_transform=True) at step 0 on the scene of test_silhouette_gpu's fit tests, checked as
    test_fit_step0_against_fp64 checks the default path: both sides evaluate the terms at the kernel's own vertices (moved32), the
    parameter gradients go through the fp64 Jacobian of the transform with its 16 u allowance (= pose.GRAD_ULPS)"""
    assert pose.GRAD_ULPS == 16
    cam, obj, faces, hum, p_obj, p_hum, offset, target, R6, T = tsg.fit_scene()
    model = fit.ObjectPoseFit(R6.to(cuda), T.to(cuda), 1.0, obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda),
                              target.to(cuda), (cam.fx, cam.fy), (cam.px, cam.py), offset.to(cuda), fused_transform=True)
    total, terms = model()
    total.sum().backward()
    assert total.shape == (2,) and set(terms) == {"mask_loss", "centroid_loss", "contact_loss"}
    moved = model.object_vertices().detach().cpu()
    # the fused vertices are the transform within the forward's documented error
    out64, _, b_out, _ = reference(obj, R6, T, 1.0, torch.zeros(2, obj.shape[0], 3))
    assert_within(moved, out64, b_out, "fused object_vertices")
    for b in range(2):
        (t64, bt), terms64, (gr, br), (gt, btr), lo = tsg._fit_step0_fp64(b, moved[b])
        assert int(lo.sum()) == 0, "choose another start: a face sits on the cut-off of the step-0 pose"
        for k, (v64, bk) in terms64.items():
            assert_within(terms[k][b], v64, torch.as_tensor(bk), f"start {b} {k}")
        assert_within(total[b], t64, torch.as_tensor(bt), f"start {b} total")
        assert_within(model.rotation.grad[b], gr, br, f"start {b} d total / d rot6d")
        assert_within(model.translation.grad[b], gt, btr, f"start {b} d total / d translation")


def _search(cuda, **kw):
    cam, obj, faces, hum, p_obj, p_hum, target, T_start = ps.search_scene()
    return fit.search_object_pose(obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda),
                                  (cam.fx, cam.fy), (cam.px, cam.py), init=(torch.eye(3), T_start, 1.0), max_iter=ps.MAX_ITER,
                                  hum_centroid_offset=None, **kw)


@functools.lru_cache(maxsize=None)
def _search_all(cuda):
    """the 24-start search without ICP, run once and shared (never modified)"""
    return _search(cuda, rotations=None, icp=False)


def test_search_finds_the_fp64_winner(hip_lib, cuda):
    res = _search_all(cuda)
    N = ps.search_scene()[1].shape[0]
    assert res["rotation"].shape == (24, 6) and res["translation"].shape == (24, 3) and res["scale"].shape == (24,)
    assert res["object_vertices"].shape == (24, N, 3) and res["history"].shape == (ps.MAX_ITER, 24) and res["scores"].shape == (24,)
    scores = res["scores"]
    print("scores:", [round(v, 4) for v in scores.tolist()])
    print(f"best {int(res['best_index'])}, scores[0] - scores[7] = {float(scores[0] - scores[7]):.4f} (fp64: 3.2350), "
          f"runner-up gap {float(scores.sort().values[1] - scores.min()):.3e} (fp64: 1.855e-02)")
    best = res["best_index"]
    assert best.dim() == 0 and best.dtype == torch.int64 and best.is_cuda
    assert int(best) == 7  # the fp64 winner (tests/golden/pose_search_fp64.json)
    assert float(scores[0] - scores[7]) > 1.0  # from the identity the fit does not get there
    assert bool(torch.isfinite(scores).all()) and torch.equal(fit.select_best(scores), best)
    assert not torch.equal(res["history"][-1], scores)  # the score is a forward at the returned parameters
    for k in ("rotation", "translation", "scale", "object_vertices"):
        assert torch.equal(res["best"][k], res[k][7])


def test_search_chunk_changes_no_bit(hip_lib, cuda):
    res, chunked = _search_all(cuda), _search(cuda, rotations=None, icp=False, chunk=5)
    for k in ("rotation", "translation", "scale", "object_vertices", "history", "scores", "best_index"):
        assert torch.equal(res[k], chunked[k]), f"{k} differs with chunk=5"
    for k, val in res["best"].items():
        assert torch.equal(val, chunked["best"][k])


@pytest.mark.parametrize("k", [0, 7, 23])
def test_search_start_equals_its_own_fit(hip_lib, cuda, k):
    res = _search_all(cuda)
    cam, obj, faces, hum, p_obj, p_hum, target, T_start = ps.search_scene()
    r6, T, s = pose.pose_starts(pose.cube_rotations()[k:k + 1].to(cuda), None, T_start.to(cuda), 1.0)
    own = fit.fit_object_pose(obj.to(cuda), faces.to(cuda), hum.to(cuda), p_obj.to(cuda), p_hum.to(cuda), target.to(cuda), (cam.fx, cam.fy),
                              (cam.px, cam.py), init=(r6, T, s), hum_centroid_offset=None, max_iter=ps.MAX_ITER, fused_transform=True)
    assert torch.equal(own["history"][:, 0], res["history"][:, k])
    for key in ("rotation", "translation", "scale", "object_vertices"):
        assert torch.equal(own[key][0], res[key][k]), f"{key} of start {k} differs from its own run"


def test_search_with_icp_runs(hip_lib, cuda):
    """icp=True: one contact_icp call moves all 24 starts first.  No pose accuracy is claimed for this leg: none is measured."""
    res = _search(cuda, rotations=None, icp=True)
    assert res["scores"].shape == (24,) and bool(torch.isfinite(res["scores"]).all())
    R = fit.rot6d_to_matrix(res["rotation"])
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, device=cuda).expand(24, 3, 3), atol=1e-5)
    best = res["best_index"]
    assert best.dim() == 0 and best.dtype == torch.int64 and best.is_cuda
    # other start sets: four turns about the up axis, scored and ranked the same way
    res4 = _search(cuda, rotations=pose.axis_rotations(4), icp=False)
    assert res4["scores"].shape == (4,) and res4["history"].shape == (ps.MAX_ITER, 4)


def test_memory_is_workspace_and_outputs(hip_lib, cuda):
    B, N = 24, 20002
    v, r6, t, s, g = make_inputs(N, B, seed=7, tensor_scale=True)
    v, g = v.to(cuda), g.to(cuda)
    leaves = [x.to(cuda).requires_grad_(True) for x in (r6, t, s)]
    ws = hip_lib.ivlm_pose_transform_workspace_bytes(B, N)
    assert 0 < ws <= B * -(-N // CH) * 96 + 256
    pose.pose_transform(v, *leaves).backward(g)  # warm: nothing is cached, but the allocator has seen the sizes
    for x in leaves:
        x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pose.pose_transform(v, *leaves).backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 12 * B * N + ws + 4 * B * (6 + 3 + 1) + (1 << 20)
    print(f"peak memory rise {rise / 1e6:.2f} MB, workspace {ws / 1e6:.3f} MB, output {12 * B * N / 1e6:.2f} MB, allowed {allowed / 1e6:.2f} MB")
    assert rise <= allowed
    assert all(bool(torch.isfinite(x.grad).all()) for x in leaves)


def test_refusals(hip_lib, cuda):
    v, r6, t, s, g = make_inputs(10, 2, seed=8, tensor_scale=True)
    vc, rc, tc, sc = (x.to(cuda) for x in (v, r6, t, s))
    for args in ((v, rc, tc, sc), (vc, r6, tc, sc), (vc, rc, t, sc), (vc, rc, tc, s)):
        with pytest.raises(IvlmError, match="GPU tensor"):
            pose.pose_transform(*args)
    for args, match in (((vc.double(), rc, tc), "float32"), ((vc, rc.half(), tc), "float32"), ((vc, rc, tc, sc.double()), "float32"),
                        ((vc[:, :2], rc, tc), r"\[N,3\]"), ((vc, rc[:, :5], tc), r"\[B,6\]"), ((vc, rc, tc[:1]), "translation"),
                        ((vc, rc, tc, torch.ones(3, device=cuda)), "scaling"), ((vc.clone().requires_grad_(True), rc, tc), "require grad")):
        with pytest.raises(ValueError, match=match):
            pose.pose_transform(*args)
    r = rc.clone().requires_grad_(True)
    out = pose.pose_transform(vc, r, tc, sc)
    (gr,) = torch.autograd.grad((out * out).sum(), r, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gr.sum().backward()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="chunk"):
            _search(cuda, icp=False, chunk=bad)
    # the C entry points refuse before any launch
    assert hip_lib.ivlm_pose_transform_workspace_bytes(1, (1 << 22) + 1) == 0
    out = torch.empty(2, 10, 3, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    assert hip_lib.ivlm_pose_transform_forward(vc.data_ptr(), rc.data_ptr(), tc.data_ptr(), sc.data_ptr(), 2, (1 << 22) + 1, out.data_ptr(), stream) == -4
    assert hip_lib.ivlm_pose_transform_forward(vc.data_ptr(), rc.data_ptr(), tc.data_ptr(), None, 2, 10, out.data_ptr(), stream) == -1
    ws = torch.empty(256, dtype=torch.uint8, device=cuda)
    assert hip_lib.ivlm_pose_transform_backward(vc.data_ptr(), rc.data_ptr(), sc.data_ptr(), out.data_ptr(), 2, 10, None, None, None, ws.data_ptr(),
                                                256, stream) == -1  # nothing asked for
    assert hip_lib.ivlm_pose_transform_backward(vc.data_ptr(), rc.data_ptr(), sc.data_ptr(), out.data_ptr(), 2, 10, None, tc.data_ptr(), None,
                                                ws.data_ptr(), 16, stream) == -2  # IVLM_ERR_WORKSPACE: too small
