"""interactvlm_amd.pose and the search helpers of interactvlm_amd.fit without a GPU: the start generators, the exact composition
of the starts, select_best, validation (which raises before the library loads), the C symbols and constants of the built library,
and the analytic Gram-Schmidt chain of the finish kernel (pose.gram_schmidt_backward, its documentation) against autograd."""
import ctypes
import itertools
import json
import math
import os

import pytest
import torch

import _pose_scene as ps
from interactvlm_amd import _lib, fit, pose
from interactvlm_amd._lib import IvlmError


@pytest.fixture(autouse=True)
def grad_enabled():
    with torch.enable_grad():
        yield


@pytest.fixture
def no_library(monkeypatch):
    """validation must raise before anything touches the library"""
    def boom():
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(_lib, "load", boom)


def test_cube_rotations():
    Q = pose.cube_rotations()
    assert Q.shape == (24, 3, 3) and Q.dtype == torch.float32
    assert len({tuple(q.reshape(-1).tolist()) for q in Q}) == 24
    assert bool(((Q == 0) | (Q == 1) | (Q == -1)).all())
    assert torch.equal(Q @ Q.transpose(1, 2), torch.eye(3).expand(24, 3, 3))
    for q in Q.tolist():  # the determinant by hand: exact on entries in {0, +-1}
        det = (q[0][0] * (q[1][1] * q[2][2] - q[1][2] * q[2][1]) - q[0][1] * (q[1][0] * q[2][2] - q[1][2] * q[2][0])
               + q[0][2] * (q[1][0] * q[2][1] - q[1][1] * q[2][0]))
        assert det == 1.0
    assert torch.equal(Q[0], torch.eye(3))
    # the documented order: permutations of (0, 1, 2) in lexicographic order, four sign triples of determinant +1 each, in the
    # order of itertools.product((1, -1), repeat=3); row i is sign[i] e_perm[i]
    assert Q[7].tolist() == [[-1, 0, 0], [0, 0, -1], [0, -1, 0]]    # perm (0, 2, 1), the last of its signs (-1, -1, -1)
    assert Q[12].tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]      # perm (1, 2, 0), even: its first signs are (1, 1, 1)
    assert Q[23].tolist() == [[0, 0, -1], [0, -1, 0], [-1, 0, 0]]   # perm (2, 1, 0), signs (-1, -1, -1)
    perms = list(itertools.permutations(range(3)))
    for k in range(24):
        assert [row.index(1.0) if 1.0 in row else row.index(-1.0) for row in Q[k].tolist()] == list(perms[k // 4])


def test_axis_rotations_closed_form():
    R = pose.axis_rotations(4)
    want = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],
            [[0, 0, -1], [0, 1, 0], [1, 0, 0]]]  # [[c, 0, s], [0, 1, 0], [-s, 0, c]] at 0, 90, 180, 270 degrees
    assert R.shape == (4, 3, 3) and R.dtype == torch.float32
    assert torch.equal(R[0], torch.eye(3))
    assert torch.allclose(R, torch.tensor(want, dtype=torch.float32), atol=2.0 ** -50, rtol=0)
    R7 = pose.axis_rotations(7, axis=(1.0, 2.0, -0.5)).double()
    a = torch.tensor([1.0, 2.0, -0.5], dtype=torch.float64)
    assert torch.allclose(R7 @ a, a.expand(7, 3), atol=1e-6)  # the axis stays
    assert torch.allclose(R7[1] @ R7[1] @ R7[1], R7[3], atol=1e-6)  # equally spaced
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="k"):
            pose.axis_rotations(bad)
    with pytest.raises(ValueError, match="axis"):
        pose.axis_rotations(3, axis=(0.0, 0.0, 0.0))


def test_pose_starts_are_exact_row_permutations():
    import _silhouette_ref as ref

    R0 = ref.random_rotation(5).float()
    T0 = torch.tensor([0.3, -0.2, 2.5])
    r6, T, s = pose.pose_starts(pose.cube_rotations(), R0, T0, 1.25)
    assert r6.shape == (24, 6) and T.shape == (24, 3) and s.shape == (24,)
    assert torch.equal(T, T0.expand(24, 3)) and torch.equal(s, torch.full((24,), 1.25))
    Rk = pose.compose_rotations(pose.cube_rotations(), R0)
    assert torch.equal(fit.matrix_to_rot6d(Rk), r6)
    bits = set(R0.reshape(-1).view(torch.int32).tolist()) | set((-R0).reshape(-1).view(torch.int32).tolist())
    assert set(Rk.reshape(-1).view(torch.int32).tolist()) <= bits  # every entry is +- an entry of R0, bit for bit
    assert torch.allclose(Rk.double(), pose.cube_rotations().double() @ R0.double(), atol=0, rtol=0)
    # the 6-D form gives the start back: 4 ulps of 1 (the entries of a rotation are at most 1)
    back = fit.rot6d_to_matrix(r6)
    assert float((back - Rk).abs().max()) <= 4 * 2.0 ** -23
    # defaults: the identity pose, so the starts are the rotations themselves
    r6, T, s = pose.pose_starts(pose.cube_rotations())
    assert torch.equal(r6, fit.matrix_to_rot6d(pose.cube_rotations())) and not bool(T.any()) and torch.equal(s, torch.ones(24))
    with pytest.raises(ValueError, match="rotations"):
        pose.pose_starts(torch.zeros(3, 3))
    with pytest.raises(ValueError, match="R0"):
        pose.pose_starts(pose.cube_rotations(), torch.zeros(3))
    with pytest.raises(ValueError, match="T0"):
        pose.pose_starts(pose.cube_rotations(), None, torch.zeros(4))


def test_select_best():
    inf, nan = float("inf"), float("nan")
    for scores, want in (([3.0, 1.5, 2.0], 1), ([2.0, 1.0, 1.0, 1.0], 1), ([nan, 4.0, -inf, 3.0, inf, 3.0], 3), ([nan, inf, -inf], 0),
                         ([5.0], 0), ([inf, -1e30, nan], 1)):
        for dtype in (torch.float32, torch.float64):
            best = fit.select_best(torch.tensor(scores, dtype=dtype))
            assert best.dim() == 0 and best.dtype == torch.int64 and int(best) == want, (scores, int(best))
    for bad in (torch.zeros(2, 2), torch.zeros(0), torch.zeros(3, dtype=torch.int64), [1.0, 2.0]):
        with pytest.raises(ValueError, match="scores"):
            fit.select_best(bad)


def test_pose_transform_refusals(no_library):
    v, r6, t = torch.zeros(5, 3), torch.zeros(2, 6), torch.zeros(2, 3)
    for bad, match in ((v.double(), "float32"), (v[:, :2], r"\[N,3\]"), (v[None], r"\[N,3\]"), (v[:0], r"\[N,3\]"), ([[0.0, 0.0, 1.0]], "tensor")):
        with pytest.raises(ValueError, match=match):
            pose.pose_transform(bad, r6, t)
    with pytest.raises(ValueError, match="must not require grad"):
        pose.pose_transform(v.clone().requires_grad_(True), r6, t)
    for bad, match in ((r6.double(), "float32"), (r6[:, :5], r"\[B,6\]"), (r6[None], r"\[B,6\]"), (None, "tensor")):
        with pytest.raises(ValueError, match=match):
            pose.pose_transform(v, bad, t)
    for bad, match in ((t.double(), "float32"), (t[:1], "translation"), (t[0], "translation"), (torch.zeros(3, 3), "translation")):
        with pytest.raises(ValueError, match=match):
            pose.pose_transform(v, r6, bad)
    with pytest.raises(ValueError, match="translation"):  # an unbatched pose takes [3]
        pose.pose_transform(v, r6[0], t)
    for bad in (torch.ones(3), torch.ones(2, 2), torch.ones(2, dtype=torch.float64), "big", float("nan")):
        with pytest.raises(ValueError, match="scaling"):
            pose.pose_transform(v, r6, t, bad)
    with pytest.raises(IvlmError, match="GPU tensor"):  # everything else in order: there is no CPU fallback
        pose.pose_transform(v, r6, t, torch.ones(2))


def test_search_object_pose_refusals(no_library):
    v, f, h = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(3, 3)
    scene = (v, f, h, torch.zeros(5), torch.zeros(3), torch.zeros(8, 8), 10.0, (4.0, 4.0))
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="chunk"):
            fit.search_object_pose(*scene, chunk=bad)
    with pytest.raises(ValueError, match="early_stop"):
        fit.search_object_pose(*scene, early_stop=True)
    with pytest.raises(ValueError, match="fused_transform"):
        fit.search_object_pose(*scene, fused_transform=False)
    with pytest.raises(ValueError, match="obj_vertices"):
        fit.search_object_pose(v[:, :2], *scene[1:])
    for bad in (torch.zeros(3, 3), torch.zeros(2, 3, 3, dtype=torch.float64), [[1.0]]):
        with pytest.raises(ValueError, match="rotations"):
            fit.search_object_pose(*scene, rotations=bad)
    for bad, match in ((torch.eye(3), "init"), ((torch.eye(3), torch.zeros(3)), "init"), ((torch.eye(4), torch.zeros(3), 1.0), "R0"), ((torch.eye(3), torch.zeros(2), 1.0), "T0"),
                       ((torch.eye(3), torch.zeros(3), "x"), "s0")):
        with pytest.raises(ValueError, match=match):
            fit.search_object_pose(*scene, init=bad)
    with pytest.raises(ValueError, match="normals"):
        fit.search_object_pose(*scene, obj_normals=v)
    with pytest.raises(ValueError, match="contact vertices"):  # icp=True with no contact above the thresholds
        fit.search_object_pose(*scene)


def test_abi_symbols_and_constants():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.header_prototypes()
    for name in ("ivlm_pose_transform_workspace_bytes", "ivlm_pose_transform_forward", "ivlm_pose_transform_backward"):
        assert name in protos, f"{name} is not declared in include/ivlm_hip.h"
        assert hasattr(lib, name), f"libivlm_hip.so does not export {name}"
    txt = open(_lib.HEADER_PATH).read()
    for const, value in (("IVLM_POSE_CHUNK", pose.POSE_CHUNK), ("IVLM_POSE_CHAIN", pose.L_CHAIN), ("IVLM_POSE_FWD_ULPS", pose.FWD_ULPS),
                         ("IVLM_POSE_GRAD_ULPS", pose.GRAD_ULPS)):
        assert f"#define {const} {value}\n" in txt, f"{const} of the header and interactvlm_amd.pose differ"
    lib.ivlm_pose_transform_workspace_bytes.restype = ctypes.c_size_t
    chunks = -(-20002 // pose.POSE_CHUNK)
    assert 24 * chunks * 96 <= lib.ivlm_pose_transform_workspace_bytes(24, 20002) <= 24 * chunks * 96 + 256
    assert lib.ivlm_pose_transform_workspace_bytes(1, (1 << 22) + 1) == 0
    assert lib.ivlm_pose_transform_workspace_bytes(65536, 10) == 0
    assert lib.ivlm_pose_transform_workspace_bytes(0, 10) == 0


@pytest.mark.parametrize("seed", range(5))
def test_gram_schmidt_chain_against_autograd(seed):
    gen = torch.Generator().manual_seed(seed)
    r6 = (torch.randn(6, generator=gen, dtype=torch.float64) * (0.3 + seed)).requires_grad_(True)
    G = torch.randn(3, 3, generator=gen, dtype=torch.float64)
    (fit.rot6d_to_matrix(r6)[0] * G).sum().backward()
    got = pose.gram_schmidt_backward(r6.detach(), G)
    assert float(r6.grad.abs().max()) > 1e-3
    assert torch.allclose(got, r6.grad, rtol=1e-12, atol=1e-12 * float(r6.grad.abs().max()))


def test_search_fixture_holds_the_margin():
    """the GPU test's winner is decided by the fp64 definitions alone: the committed finals keep winner and runner-up apart by at
    least 1e-3 of the winning total, and the identity start more than 1.0 behind"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ps.GOLDEN)) as f:
        gold = json.load(f)
    finals = gold["final_total"]
    order = sorted(range(24), key=lambda k: finals[k])
    assert len(finals) == 24 and all(math.isfinite(v) for v in finals)
    assert order[0] == ps.TRUE_INDEX == gold["winner"] and gold["max_iter"] == ps.MAX_ITER
    assert finals[order[1]] - finals[order[0]] >= 1e-3 * finals[order[0]]
    assert finals[0] - finals[ps.TRUE_INDEX] > 1.0
    cam, obj, faces, hum, p_obj, p_hum, target, _ = ps.search_scene()
    assert (obj.shape[0], faces.shape[0], int((p_obj > 0).sum()), int((p_hum > 0).sum()), int(target.sum())) == (86, 168, 15, 9, 205)
    assert (gold["vertices"], gold["faces"], gold["contact_obj"], gold["contact_hum"], gold["target_pixels"]) == (86, 168, 15, 9, 205)
    # the fixture is what the fp64 loop gives: one start re-run (a second of CPU)
    history, final = ps.fit_fp64(ps.TRUE_INDEX)
    assert final == pytest.approx(finals[ps.TRUE_INDEX], rel=1e-9) and history[0] == pytest.approx(gold["first_total"][ps.TRUE_INDEX], rel=1e-9)
