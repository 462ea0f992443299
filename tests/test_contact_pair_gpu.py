"""contact_distance (csrc/contact_pair.hip) against its definition written in torch fp64 on the CPU:

    d_ij = |o_i - h_j|,  S = (sum p)(sum q),  L = sum_ij p_i q_j d_ij / S
    dL/do_i = (p_i / S) sum_j q_j (o_i - h_j) / d_ij,   dL/dh_j = -(q_j / S) sum_i p_i (o_i - h_j) / d_ij   (0 where d_ij == 0)

Tolerances are derived, not tuned: with u = 2^-24 and c = L_CHAIN + 8 (the kernel's documented longest serial fp32
accumulation + the roundings of one term), |L - L64| <= c u L64 (all terms are non-negative) and |g - g64| <= c u A with A the
same sum over the absolute values of the terms, in fp64.
"""
import functools

import pytest
import torch

from interactvlm_amd import contact_pair as cp
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C = cp.L_CHAIN + 8


@pytest.fixture(autouse=True)
def grad_enabled():
    """These tests differentiate, and a whole-suite run reaches them with autograd switched off for the process:
    tests/test_oracle_nn.py calls torch.set_grad_enabled(False) at import (collection time), and so do the model fixtures of
    test_heads_gpu, test_model_gpu, test_parity_mode_gpu, test_speculative_gpu, test_exact_sets_gpu and test_fp8_gpu.  The hazard
    belongs fixed there (a scoped torch.no_grad()); until then this file sets and restores the mode it needs."""
    with torch.enable_grad():
        yield


def make_inputs(n_o, n_h, seed=0, batch_o=None, batch_h=None, density=0.1):
    g = torch.Generator().manual_seed(seed * 1000003 + n_o * 7919 + n_h)
    o = torch.randn(*([batch_o] if batch_o else []), n_o, 3, generator=g)
    h = torch.randn(*([batch_h] if batch_h else []), n_h, 3, generator=g)

    def probs(n, side):
        if isinstance(density, tuple):  # (m_o, m_h): exactly m non-zero entries - the last vertex, from m = 2 on the first, the rest anywhere
            keep = torch.zeros(n, dtype=torch.bool)
            keep[[0, n - 1][-density[side]:]] = True
            keep[1 + torch.randperm(max(n - 2, 0), generator=g)[:max(density[side] - 2, 0)]] = True
            return (0.05 + torch.rand(n, generator=g)) * keep
        p = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < density)
        if not bool((p > 0).any()):  # S == 0 is NaN by definition and not a case here: keep one contact vertex
            p[int(torch.randint(n, (1,), generator=g))] = 0.5
        return p

    return o, h, probs(n_o, 0), probs(n_h, 1)


def definition64(o, h, p, q):
    """-> L, dL/do, dL/dh and the absolute sums A_o, A_h of the gradient terms, all fp64 on the CPU (unbatched inputs)"""
    o, h, p, q = (t.detach().cpu().double() for t in (o, h, p, q))
    diff = o[:, None, :] - h[None, :, :]
    d = diff.norm(dim=-1)
    w = p[:, None] * q[None, :]
    S = p.sum() * q.sum()
    L = (w * d).sum() / S
    unit = torch.where(d[..., None] > 0, diff / d[..., None].clamp_min(1e-300), torch.zeros_like(diff))
    t = w[..., None] * unit / S
    return L, t.sum(1), -t.sum(0), t.abs().sum(1), t.abs().sum(0)


@functools.lru_cache(maxsize=None)
def case(n_o, n_h, density=0.1):
    """inputs (CPU) and the fp64 definition, computed once per shape and shared by the tests; never modified"""
    inp = make_inputs(n_o, n_h, density=density)
    return inp, definition64(*inp)


# The kernel tiles the COMPACTED lists (m = number of non-zero probabilities), so a shape reaches a tile boundary only through m.
# The issue's four shapes at 90 % zeros compact to a single tile and a single stationary block per side; the same definition and
# bound at density 1 (m = N) put m on and next to the tile of 512 and the stationary block / fold block of 256:
#   (1025, 1024)  object: 5 stationary blocks, 5 fold blocks, 3 tiles with a tail of 1; human: exactly 2 full tiles
#   (257, 6890)   human: 14 tiles, 27 stationary blocks; object: a stationary block of 1
#   (512, 513) and (513, 512)  one full tile exactly, and one full tile followed by a 1-entry tail, on either side
#
# The compaction itself (one block of 1024 threads per side, a segment of ceil(N / 1024) vertices per thread) has its edges in N:
# 1 (one thread has work; (1, 1) above), 1023 (segments of 1, the last thread idle), 1025 (segments of 2, half the threads idle).  A
# density (m_o, m_h) asks for exactly that many non-zero probabilities, the first and the last vertex among them (a single one is the
# last): m = 1, and 256 / 257 = one fold block of object vertices exactly and one more.
SHAPES = [(70, 33, 0.1), (257, 6890, 0.1), (1, 1, 0.1), (1025, 1024, 0.1),
          (1025, 1024, 1.0), (257, 6890, 1.0), (512, 513, 1.0), (513, 512, 1.0),
          (1023, 1025, (256, 257)), (1025, 1023, (257, 256)), (1023, 1025, (1, 1)), (1, 1023, (1, 257))]


def run(dev, o, h, p, q, grads=True):
    """-> (L, dL/do | None, dL/dh | None) from the code under test; gradients of sum(L)"""
    o = o.detach().to(dev).clone().requires_grad_(grads)
    h = h.detach().to(dev).clone().requires_grad_(grads)
    L = cp.contact_distance(o, h, p.to(dev), q.to(dev))
    if grads:
        L.sum().backward()
    return L.detach(), o.grad, h.grad


def assert_within(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: error exceeds the derived bound by {worst:.3e}"


@pytest.mark.parametrize("n_o,n_h,density", SHAPES)
def test_value_and_both_gradients(hip_lib, cuda, n_o, n_h, density):
    (o, h, p, q), (L64, go64, gh64, Ao, Ah) = case(n_o, n_h, density)
    if density == 1.0:  # the compacted counts are the shape itself: the boundaries named above are really reached
        assert int((p != 0).sum()) == n_o and int((q != 0).sum()) == n_h
    if isinstance(density, tuple):
        assert (int((p != 0).sum()), int((q != 0).sum())) == density and bool(p[-1] != 0) and bool(q[-1] != 0)
        assert all(bool(w[0] != 0) for w, m in ((p, density[0]), (q, density[1])) if m >= 2)
    L, go, gh = run(cuda, o, h, p, q)
    assert L.shape == () and go.shape == (n_o, 3) and gh.shape == (n_h, 3)
    assert_within(L, L64, C * U * L64, "L")
    assert_within(go, go64, C * U * Ao, "dL/do")
    assert_within(gh, gh64, C * U * Ah, "dL/dh")
    # forward only (no gradient outputs asked of the kernel): the same value
    assert torch.equal(run(cuda, o, h, p, q, grads=False)[0], L)


@pytest.mark.parametrize("n_o,n_h", [(70, 33), (1025, 1024), (7000, 6890)])
def test_sparsity_skip_is_exact(hip_lib, cuda, n_o, n_h):
    o, h, p, q = make_inputs(n_o, n_h)
    ko, kh = p != 0, q != 0
    assert int(ko.sum()) < n_o or int(kh.sum()) < n_h
    if n_o == 7000:  # the compacted lists span more than one tile and stationary block on both sides
        assert int(ko.sum()) > 512 and int(kh.sum()) > 512
    L, go, gh = run(cuda, o, h, p, q)
    Lc, goc, ghc = run(cuda, o[ko], h[kh], p[ko], q[kh])
    assert torch.equal(L, Lc)
    assert torch.equal(go[ko.to(cuda)], goc) and torch.equal(gh[kh.to(cuda)], ghc)
    assert not bool(go[~ko.to(cuda)].any()) and not bool(gh[~kh.to(cuda)].any())


# (600, 520) with every probability non-zero: 3 object fold blocks per pose (the per-pose block sums), 2 tiles on either side
@pytest.mark.parametrize("n_o,n_h,density", [(70, 33, 0.1), (600, 520, 1.0)])
@pytest.mark.parametrize("batched", ["object", "human"])
def test_batch_and_broadcast(hip_lib, cuda, batched, n_o, n_h, density):
    B = 3
    o, h, p, q = make_inputs(n_o, n_h, seed=1, batch_o=B if batched == "object" else None,
                             batch_h=B if batched == "human" else None, density=density)
    L, go, gh = run(cuda, o, h, p, q)
    assert L.shape == (B,)
    singles = [run(cuda, o[b] if batched == "object" else o, h[b] if batched == "human" else h, p, q) for b in range(B)]
    assert torch.equal(L, torch.stack([s[0] for s in singles]))
    go1, gh1 = torch.stack([s[1] for s in singles]), torch.stack([s[2] for s in singles])
    # the batched side gets its per-pose gradient, the shared side the sum over the poses
    assert torch.equal(go, go1 if batched == "object" else go1.sum(0))
    assert torch.equal(gh, gh1 if batched == "human" else gh1.sum(0))
    # the last pose against the fp64 definition (the per-pose gradients: those of the singles, which are the same bits)
    b = B - 1
    L64, go64, gh64, Ao, Ah = definition64(o[b] if batched == "object" else o, h[b] if batched == "human" else h, p, q)
    assert_within(L[b], L64, C * U * L64, "L")
    assert_within(go1[b], go64, C * U * Ao, "dL/do")
    assert_within(gh1[b], gh64, C * U * Ah, "dL/dh")


def test_reproducible(hip_lib, cuda):
    (o, h, p, q), _ = case(257, 6890)
    a, b = run(cuda, o, h, p, q), run(cuda, o, h, p, q)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _rigid(verts, theta):
    """axis-angle theta[:3] (Rodrigues) and translation theta[3:] applied to verts [N,3]"""
    w, t = theta[:3], theta[3:]
    ang = w.norm()
    k = w / ang
    zero = torch.zeros((), dtype=theta.dtype, device=theta.device)
    K = torch.stack([torch.stack([zero, -k[2], k[1]]), torch.stack([k[2], zero, -k[0]]), torch.stack([-k[1], k[0], zero])])
    R = torch.eye(3, dtype=theta.dtype, device=theta.device) + torch.sin(ang) * K + (1 - torch.cos(ang)) * (K @ K)
    return verts @ R.T + t


def test_autograd_through_rigid_transform(hip_lib, cuda):
    (o, h, p, q), _ = case(70, 33)
    theta0 = torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4, 0.25])
    # fp64 CPU autograd of the definition
    th64 = theta0.double().requires_grad_(True)
    o64, h64, p64, q64 = o.double(), h.double(), p.double(), q.double()
    d64 = (_rigid(o64, th64)[:, None, :] - h64[None, :, :]).norm(dim=-1)
    L64 = (p64[:, None] * q64[None, :] * d64).sum() / (p64.sum() * q64.sum())
    L64.backward()
    # the per-vertex bound of the first test at the transformed vertices, propagated through |Jacobian|
    moved = _rigid(o64, th64.detach())
    _, _, _, Ao, _ = definition64(moved, h, p, q)
    J = torch.autograd.functional.jacobian(lambda th: _rigid(o64, th), th64.detach())  # [N_o, 3, 6]
    bound = (J.abs() * (C * U * Ao)[..., None]).sum((0, 1))
    # the code under test: an nn.Parameter holding rotation and translation, as the fitter uses it
    theta = torch.nn.Parameter(theta0.to(cuda))
    L = cp.contact_distance(_rigid(o.to(cuda), theta), h.to(cuda), p.to(cuda), q.to(cuda))
    L.backward()
    assert theta.grad is not None and theta.grad.shape == (6,)
    assert_within(L, L64.detach(), C * U * L64.detach(), "L")
    assert_within(theta.grad, th64.grad, bound, "dL/dtheta")


def test_coincident_points(hip_lib, cuda):
    (o, h, p, q), _ = case(70, 33)
    o, p, q = o.clone(), p.clone(), q.clone()
    o[3] = h[5]
    p[3], q[5] = 0.75, 0.5
    L64, go64, gh64, Ao, Ah = definition64(o, h, p, q)  # (the definition masks d == 0 pairs)
    L, go, gh = run(cuda, o, h, p, q)
    assert bool(torch.isfinite(go).all()) and bool(torch.isfinite(gh).all()) and bool(torch.isfinite(L))
    assert_within(L, L64, C * U * L64, "L")
    assert_within(go, go64, C * U * Ao, "dL/do")
    assert_within(gh, gh64, C * U * Ah, "dL/dh")
    # only the coincident pair: both gradients are exactly zero
    one = torch.ones(1)
    _, g1, g2 = run(cuda, h[5:6].clone(), h[5:6].clone(), one, one)
    assert not bool(g1.any()) and not bool(g2.any())


def test_no_dense_intermediate(hip_lib, cuda):
    n_o, n_h = 4096, 6890
    o, h, p, q = make_inputs(n_o, n_h, seed=2, density=1.0)  # every vertex in contact: the largest workspace
    o, h = o.to(cuda).requires_grad_(True), h.to(cuda).requires_grad_(True)
    p, q = p.to(cuda), q.to(cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    cp.contact_distance(o, h, p, q).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak memory rise {rise / 1e6:.2f} MB (a dense fp32 [N_o,N_h] array: {n_o * n_h * 4 / 1e6:.0f} MB)")
    assert rise < 8e6
    assert bool(torch.isfinite(o.grad).all()) and bool(torch.isfinite(h.grad).all())


def test_refusals(hip_lib, cuda):
    lib = hip_lib
    (o, h, p, q), _ = case(70, 33)
    od, hd, pd, qd = (t.to(cuda) for t in (o, h, p, q))
    nbytes = lib.ivlm_contact_pair_workspace_bytes(1, 70, 33)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    val = torch.empty(1, device=cuda)
    good = [od.data_ptr(), hd.data_ptr(), pd.data_ptr(), qd.data_ptr(), 0, 1, 70, 33, 0, 0, val.data_ptr(), None, None,
            ws.data_ptr(), nbytes, None]
    for i in (0, 1, 2, 3, 10, 13):  # a null pointer
        bad = list(good)
        bad[i] = None
        assert lib.ivlm_contact_pair(*bad) == -1
    for i in (5, 6, 7):  # a non-positive size
        for v in (0, -1):
            bad = list(good)
            bad[i] = v
            assert lib.ivlm_contact_pair(*bad) == -1
    bad = list(good)
    bad[4] = 4  # fp16 probabilities are not handled
    assert lib.ivlm_contact_pair(*bad) == -4
    bad = list(good)
    bad[14] = nbytes - 1
    assert lib.ivlm_contact_pair(*bad) == -2
    with pytest.raises((IvlmError, ValueError)):
        cp.contact_distance(od, hd, pd[:-1], qd)
    with pytest.raises((IvlmError, ValueError)):
        cp.contact_distance(od, hd, pd, torch.cat([qd, qd]))
    with pytest.raises((IvlmError, ValueError)):
        cp.contact_distance(o, h, p, q)
    with pytest.raises((IvlmError, ValueError)):
        cp.contact_distance(od, h, pd, qd)


def test_bf16_probabilities(hip_lib, cuda):
    (o, h, p, q), _ = case(257, 6890)
    pb, qb = p.bfloat16(), q.bfloat16()
    assert bool((pb != 0).any()) and bool((qb != 0).any())
    a = run(cuda, o, h, pb, qb)
    b = run(cuda, o, h, pb.float(), qb.float())
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_mixed_probability_dtypes_are_upcast(hip_lib, cuda):
    (o, h, p, q), _ = case(257, 6890)
    pb = p.bfloat16()
    a = run(cuda, o, h, pb, q)
    b = run(cuda, o, h, pb.float(), q)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_double_backward_raises(hip_lib, cuda):
    (o, h, p, q), _ = case(70, 33)
    od = o.to(cuda).requires_grad_(True)
    L = cp.contact_distance(od, h.to(cuda), p.to(cuda), q.to(cuda))
    # L * L: the incoming gradient 2 L depends on the input, so a graph through backward exists and would treat dL/do as constant
    (g,) = torch.autograd.grad(L * L, od, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_contact_agreement_takes_evaluate_results(hip_lib, cuda):
    (o, h, p, q), (L64, *_rest) = case(70, 33)
    out_h = {"pred_contact_3d": q.to(cuda)[None]}
    out_o = {"pred_contact_3d": p.to(cuda)[None]}
    L = cp.contact_agreement(out_h, out_o, h.to(cuda), o.to(cuda))
    assert_within(L, L64, C * U * L64, "L")
