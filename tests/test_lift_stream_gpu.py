"""The streaming (pixel-major) lift kernels on the paths the golden-vector tests do not reach: vote tables above the 64 KB of LDS
a kernel gets without asking (the raised cap), the largest table the LDS budget admits and the first one past it (global atomics),
and several slabs per view summed by lift_finalize_kernel.

Their LDS / L2 float atomics commit in no fixed order, so the sums are compared with the plan gather of the same tables - which is
pinned bit for bit by test_lift_bits_gpu.py - under the atol = 2e-6 that test_lift_gpu.py::test_edge_cases uses for this comparison;
the visibility counts are compared exactly.  Measured on an MI355X at commit 0c4d1fe, before the kernels' frame and launcher were
folded: the worst difference over the cases below was 1.8e-7 (mesh, B = 3, thresholded) and 1.2e-7 (points), so 2e-6 holds as stated.

These are black-box tests: they compare results only.  The sizes 20352 and 20353 make sure that both sides of the launcher's LDS
threshold are run and give the right sums, whichever path the launcher takes for them; they do not pin where the threshold lies."""
import numpy as np
import pytest
import torch

from interactvlm_amd import ops, synth

pytestmark = pytest.mark.gpu

ATOL = 2e-6
V = 4
LDS_EDGE = (160 * 1024 - 1024) // 8  # 20352 vertices: two fp32 tables of that length fill the streaming kernels' LDS budget


def _dev(a, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return t.to(dtype) if dtype is not None else t


def _mesh(dev, B, H, W, nv, mode, param):
    vid, bary = synth.synth_mesh_tables(V, H, W, nv, fg=0.4, seed=1)
    vid, bary = _dev(vid, dev, torch.int32), _dev(bary, dev)
    logits = _dev(synth.synth_normal("lift_stream/mesh", (B, V, H, W), 3.0, seed=nv), dev)
    want, want_n = ops.lift_mesh_plan(logits, ops.LiftPlan(vid, bary, nv), mode, param, want_nviews=True)
    got, got_n = ops.lift_mesh_dense(logits, vid, bary, nv, mode, param, want_nviews=True)
    print(f"lift_mesh_dense B={B} {H}x{W} nv={nv} mode={mode}: max|d| = {(got - want).abs().max().item():.3e}")
    assert want_n.any() and torch.equal(got_n, want_n)
    assert torch.allclose(got, want, atol=ATOL, rtol=0)


def _points(dev, B, H, W, n):
    pid = _dev(synth.synth_point_maps(1, V, H, W, n, fg=0.5, seed=1)[0], dev, torch.int32)
    probs = _dev(synth.synth_uniform("lift_stream/points", (B, V, H, W), 0, 1, seed=n), dev)
    want, want_n = ops.lift_points_plan(probs, ops.LiftPlan.from_points(pid, n), want_nviews=True)
    got, got_n = ops.lift_points(probs, pid, n, want_nviews=True)
    print(f"lift_points B={B} {H}x{W} np={n}: max|d| = {(got - want).abs().max().item():.3e}")
    assert want_n.any() and torch.equal(got_n, want_n)
    assert torch.allclose(got, want, atol=ATOL, rtol=0)


@pytest.mark.parametrize("nv", [9000, LDS_EDGE, LDS_EDGE + 1])
def test_mesh_dense_around_the_lds_cap(hip_lib, cuda, nv):
    """72 000 B of LDS (above the default 64 KB), the largest table the LDS budget admits, the first one past it"""
    _mesh(cuda, 1, 32, 32, nv, 0, 20.0)


def test_points_above_the_default_lds(hip_lib, cuda):
    _points(cuda, 1, 32, 32, 9000)


@pytest.mark.parametrize("B", [1, 3])
def test_several_slabs_per_view(hip_lib, cuda, B):
    """128 x 128 pixels are four blocks of 1024 threads x 4 pixels per view: four slabs for lift_finalize_kernel to sum"""
    _mesh(cuda, B, 128, 128, 997, 0, 20.0)
    _mesh(cuda, B, 128, 128, 997, 1, 0.3)
    _points(cuda, B, 128, 128, 997)
