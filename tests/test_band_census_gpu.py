"""The band census kernels (csrc/census.hip) against NumPy: exact integer counts, bit-equal minimum distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = (0.5, 0.3)
MARGIN = 1e-3


def _contact_case(B, nv, seed):
    """uniform [0, 1) values with planted entries, spread over the rows as far as they fit: t, t +- margin as fp32 computes them, the
    next fp32 after t + margin (just outside the band), a NaN and an inf"""
    rng = np.random.default_rng(seed)
    p = rng.random((B, nv), dtype=np.float32)
    m = np.float32(MARGIN)
    plants = []
    for t in THR:
        t = np.float32(t)
        plants += [t, np.float32(t + m), np.float32(t - m), np.nextafter(np.float32(t + m), np.float32(2.0))]
    plants += [np.float32("nan"), np.float32("inf")]
    pos = rng.permutation(B * nv)[: len(plants)]
    for k, i in enumerate(pos):  # (B * nv = 1: only the first plant, 0.5 itself)
        p.reshape(-1)[i] = plants[k]
    return p


def _contact_ref(p, thr, margin):
    thr = np.asarray(thr, np.float32)
    fin = np.isfinite(p)
    d = np.abs(p[:, :, None] - thr[None, None, :]).astype(np.float32)  # fp32 subtraction, as the kernel's
    assert d.dtype == np.float32
    counts = np.concatenate([((d <= np.float32(margin)) & fin[:, :, None]).sum(1), (~fin).sum(1)[:, None]], 1).astype(np.int32)
    mind = np.where(fin[:, :, None], d, np.float32("inf")).min(1).astype(np.float32)
    return counts, mind


@pytest.mark.parametrize("B,nv,ld", [(3, 257, 257), (1, 1, 1), (2, 6890, 6890), (1, 6890, 6890), (4, 2048, 2051), (4, 2048, 2052)])
def test_contact_band_census_vs_numpy(hip_lib, cuda, B, nv, ld):
    """Counts, non-finite counts and minimum distances of every row equal NumPy's (distances bit for bit, the difference taken in
    fp32 on both sides); a second call is bit-identical; margin 0 counts exact hits only.  ld > Nv: rows of a wider buffer, with a
    stride that breaks (2051) and one that keeps (2052) the 16-byte alignment of the rows - both load paths; (1, 6890) is the shape of
    a call's own contact map (16-byte loads with a 2-element tail)."""
    import torch

    from interactvlm_amd import ops

    p = _contact_case(B, nv, seed=B * 100003 + nv)
    buf = torch.full((B, ld), 0.5, dtype=torch.float32)  # (the padding columns sit ON a threshold: they must not be counted)
    buf[:, :nv] = torch.from_numpy(p)
    dev = buf.to(cuda)[:, :nv]
    assert dev.stride(0) == ld or B == 1
    for margin in (MARGIN, 0.0):
        exp_c, exp_d = _contact_ref(p, THR, margin)
        c, d = ops.contact_band_census(dev, THR, margin)
        c2, d2 = ops.contact_band_census(dev, torch.tensor(THR, dtype=torch.float32, device=cuda), margin)
        assert c.dtype == torch.int32 and c.shape == (B, 3) and d.dtype == torch.float32 and d.shape == (B, 2)
        assert np.array_equal(c.cpu().numpy(), exp_c), (c.cpu().numpy(), exp_c)
        assert np.array_equal(d.cpu().numpy().view(np.uint32), exp_d.view(np.uint32))
        assert torch.equal(c, c2) and torch.equal(d.view(torch.int32), d2.view(torch.int32))
    if B * nv > 16:  # the planted values did what they were planted for
        exp_c, _ = _contact_ref(p, THR, MARGIN)
        exp_0, _ = _contact_ref(p, THR, 0.0)
        assert exp_0[:, :2].sum() >= 2 and exp_c[:, 2].sum() == 2
        assert (exp_0[:, :2].sum(0) < exp_c[:, :2].sum(0)).all()


def test_contact_band_census_rows_without_finite_values_and_bad_arguments(hip_lib, cuda):
    import torch

    from interactvlm_amd import _lib, ops

    p = torch.tensor([[float("nan"), float("inf"), -float("inf")], [0.5, 0.25, 1.0]], device=cuda)
    c, d = ops.contact_band_census(p, (0.5,), 0.0)
    assert c.tolist() == [[0, 3], [1, 0]] and d.tolist() == [[float("inf")], [0.0]]
    with pytest.raises(_lib.IvlmError):
        ops.contact_band_census(p.cpu(), (0.5,), 0.0)
    with pytest.raises(_lib.IvlmError):
        ops.contact_band_census(p, (0.1, 0.2, 0.3, 0.4, 0.5), 0.0)
    with pytest.raises(_lib.IvlmError):
        ops.contact_band_census(p, (0.5,), -1.0)
    with pytest.raises(_lib.IvlmError):
        ops.contact_band_census(p.double(), (0.5,), 0.0)


def test_mask_band_census_vs_numpy(hip_lib, cuda):
    """A small plan built by ops.LiftPlan from a random table (V = 2, 64 x 64, Nv = 257, 40 % foreground), logits N(0, 4^2) with
    pixels planted at logit(0.3) inside and outside the plan: the number of plan ENTRIES in the band equals NumPy's walk over the
    tables (one entry per corner of a valid triple); pixels outside the plan are never counted; non-finite logits are counted apart.
    The device's expf and NumPy's exp may differ in the last bits: the reference must not have a value that close to the band's
    edge (asserted), so the comparison is exact."""
    import torch

    from interactvlm_amd import _lib, ops, synth

    V, H, W, nv = 2, 64, 64, 257
    thr, margin = np.float32(0.3), np.float32(1e-3)
    vid, bary = synth.synth_mesh_tables(V, H, W, nv, fg=0.4, seed=5)
    vid = np.asarray(vid).astype(np.int32)
    valid = ((vid >= 0) & (vid < nv)).all(-1)  # the plan builder's rule: all three ids in range
    per_pixel = 3 * valid.astype(np.int64)  # entries per pixel
    rng = np.random.default_rng(11)
    logits = (4.0 * rng.standard_normal((V, H, W))).astype(np.float32)
    x03 = np.float32(np.log(0.3 / 0.7))
    inside, outside = np.argwhere(valid), np.argwhere(~valid)
    assert len(inside) > 100 and len(outside) > 100
    pick_in = inside[rng.permutation(len(inside))[:7]]
    pick_out = outside[rng.permutation(len(outside))[:9]]
    for v, y, x in np.concatenate([pick_in, pick_out]):
        logits[v, y, x] = x03
    bad_in, bad_out = inside[rng.permutation(len(inside))[-1]], outside[rng.permutation(len(outside))[-1]]
    logits[tuple(bad_in)] = np.float32("nan")
    logits[tuple(bad_out)] = np.float32("inf")

    fin = np.isfinite(logits)
    with np.errstate(invalid="ignore", over="ignore"):
        sig = (np.float32(1.0) / (np.float32(1.0) + np.exp(-logits))).astype(np.float32)
        dist = np.abs(sig - thr)
    assert not (fin & (np.abs(dist - margin) < 1e-6)).any()  # nothing within a few ulp of the band's edge
    in_band = fin & (dist <= margin)
    exp = [int((per_pixel * in_band).sum()), int((per_pixel * ~fin).sum())]
    assert exp[0] >= 3 * 7 and exp[1] == 3
    assert int((in_band & ~valid).sum()) >= 9  # band pixels outside the plan exist, and count for nothing

    plan = ops.LiftPlan(torch.from_numpy(vid).to(cuda), torch.from_numpy(np.asarray(bary, np.float32)).to(cuda), nv)
    assert plan.nnz == int(per_pixel.sum())
    lg = torch.from_numpy(logits).to(cuda)
    c = ops.mask_band_census(lg, plan, 0.3, 1e-3)
    assert c.dtype == torch.int32 and c.tolist() == exp
    assert torch.equal(ops.mask_band_census(lg[None], plan, 0.3, 1e-3), c)  # [1,V,H,W], and reproducible
    # only the plan's pixels: with every plan pixel moved far from the threshold, the planted outside pixels alone count nothing
    far = logits.copy()
    far[valid] = 8.0
    assert ops.mask_band_census(torch.from_numpy(far).to(cuda), plan, 0.3, 1e-3).tolist() == [0, 0]
    # a margin of 1 takes every entry with a finite logit
    assert ops.mask_band_census(lg, plan, 0.3, 1.0).tolist() == [int(per_pixel.sum()) - 3, 3]
    with pytest.raises(_lib.IvlmError):
        ops.mask_band_census(lg.cpu(), plan, 0.3, 1e-3)
    with pytest.raises(_lib.IvlmError):
        ops.mask_band_census(lg[:1].contiguous(), plan, 0.3, 1e-3)
