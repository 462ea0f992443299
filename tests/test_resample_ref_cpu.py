"""The float64 resampling reference and its derived bound (tests/_resample_ref.py), checked without a GPU: the reference is torch's
float64 bilinear interpolate, the bound admits a correct fp32 evaluation (torch's, and the two fp32 oracles) and rejects a one-tap
error by at least two orders of magnitude."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resample_ref as R

KINDS = ("smooth", "ramp", "impulse")
REJECT = 100.0  # a one-pixel shift of the input must miss the bound by at least this factor


def _input(kind, case):
    h, w = case[:2]
    if kind == "impulse":  # one the output is sure to sample, two corners
        return np.stack([R.impulse(h, w, *R.visible_impulse(case)), R.impulse(h, w, 0, w - 1), R.impulse(h, w, h - 1, 0)])
    return R.make_input(kind, R.N_IMAGES, h, w)


def _torch_post(low, img, ins, orig, dtype):
    t = torch.from_numpy(np.array(low)).to(dtype)[:, None]
    t = F.interpolate(t, (img, img), mode="bilinear", align_corners=False)[..., : ins[0], : ins[1]]
    if tuple(ins) != tuple(orig):
        t = F.interpolate(t, tuple(orig), mode="bilinear", align_corners=False)
    return t[:, 0].double().numpy()


@pytest.mark.parametrize("case", R.POST_CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
def test_post64_is_torch_float64(case, kind):
    h, w, img, ins, orig = case
    low = _input(kind, case)
    ref = R.post64(low, img, ins, orig)
    assert ref.shape == (low.shape[0],) + tuple(orig) and ref.dtype == np.float64
    scale = max(1.0, float(np.abs(low).max()))  # (the ramp reaches 3e4: 1e-12 relative to the largest input)
    np.testing.assert_allclose(ref, _torch_post(low, img, ins, orig, torch.float64), atol=1e-12 * scale, rtol=0)


@pytest.mark.parametrize("case", R.POST_CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
def test_bound_admits_fp32_and_rejects_a_one_pixel_shift(case, kind):
    from oracle import cref, lift

    h, w, img, ins, orig = case
    low = _input(kind, case)
    ref, e = R.post64(low, img, ins, orig), R.bound(low, img, ins, orig)
    assert e.shape == (low.shape[0], 1, 1) and (e[np.abs(low).max(axis=(1, 2)) > 0] > 0).all()
    for name, got in (("torch fp32", _torch_post(low, img, ins, orig, torch.float32)),
                      ("oracle/cref", cref.postprocess_masks(low[:, None], ins, orig, img)[:, 0].astype(np.float64)),
                      ("oracle/lift", lift.postprocess_masks(low[:, None], ins, orig, img)[:, 0].astype(np.float64))):
        ratio = R.worst(np.abs(got - ref), e)
        assert ratio <= 1.0, f"{name}: err / bound = {ratio:.3g}"
    for axis in (1, 2):
        if low.shape[axis] == 1:  # (a one-pixel axis has nothing to shift)
            continue
        off = R.worst(np.abs(R.post64(np.roll(low, 1, axis=axis), img, ins, orig) - ref), e)
        assert off >= REJECT, f"a shift along axis {axis} is only {off:.3g} x the bound"


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", ("smooth", "ramp", "smooth24"))
def test_resize64_bound_and_bf16_window(case, kind):
    (h, w), (oh, ow) = case
    src = R.make_input(kind, R.N_IMAGES, h, w)
    ref, e = R.resize64(src, oh, ow), R.bound(src)
    t = torch.from_numpy(np.array(src))[:, None]
    np.testing.assert_allclose(ref, F.interpolate(t.double(), (oh, ow), mode="bilinear", align_corners=False)[:, 0].numpy(),
                               atol=1e-12 * max(1.0, float(np.abs(src).max())), rtol=0)
    got = F.interpolate(t, (oh, ow), mode="bilinear", align_corners=False)[:, 0]
    assert float((np.abs(got.double().numpy() - ref) / e).max()) <= 1.0
    # the condition of the bf16 test: the window of a stored value holds ONE bf16 value for all but a few pixels - and torch's own
    # bf16 store of its fp32 result lies inside it
    lo, hi = R.bf16_window(ref, e)
    g16 = got.to(torch.bfloat16).double().numpy()
    assert ((g16 >= lo) & (g16 <= hi)).all()
    print(f"{kind} {R.case_id(case)}: windows of two bf16 values {float((lo != hi).mean()):.4f}")
    if kind == "smooth24":  # (the input of the bf16-output GPU test; an output of three pixels may hold one such window)
        assert int((lo != hi).sum()) <= max(1, int(R.BF16_STRADDLE_MAX * lo.size)), float((lo != hi).mean())
    for axis in (1, 2):
        off = np.abs(R.resize64(np.roll(src, 1, axis=axis), oh, ow) - ref) / e
        assert float(off.max()) >= REJECT


def test_bf16_windows_hold_one_value():
    """over all pixels of the bf16-output test at most 2 % have a window of two bf16 values: the test pins the stored bits"""
    two = total = 0
    for (h, w), (oh, ow) in R.RESIZE_CASES:
        src = R.make_input("smooth24", R.N_IMAGES, h, w)
        lo, hi = R.bf16_window(R.resize64(src, oh, ow), R.bound(src))
        two, total = two + int((lo != hi).sum()), total + lo.size
    assert two / total <= R.BF16_STRADDLE_MAX, two / total


def test_sigmoid_bound_and_inputs():
    low = R.smooth(3, 16, 12)
    e, es = R.bound(low, 64, (64, 43), (5, 1027)), R.bound(low, 64, (64, 43), (5, 1027), sigmoid=True)
    np.testing.assert_array_equal(es, e / 4.0 + 1e-6)
    assert (R.bound(low, 64, (64, 43), (64, 43)) < e).all()  # the identity second resize has no second coordinate term
    # inputs: amplitudes, frequency, asymmetry, the bf16 rounding of the ramp is exact up to 256
    assert low.dtype == np.float32 and 1.0 < np.abs(low).max() <= 12.0 and not np.array_equal(low[0], low[1])
    big = R.smooth(1, 64, 64)[0].astype(np.float64)
    spec = np.abs(np.fft.fft2(big * np.outer(np.hanning(64), np.hanning(64))))
    fy, fx = np.meshgrid(np.fft.fftfreq(64), np.fft.fftfreq(64), indexing="ij")
    assert spec[np.hypot(fy, fx) > 0.16].max() < 1e-2 * spec.max()
    r = R.ramp(3, 4, 5)
    assert r[2, 3, 4] == 2304.0 and r[1, 0, 0] == 1000.0 and r[0, 1, 0] == 100.0 and r[0, 0, 1] == 1.0
    assert R.impulse(4, 5, 3, 1).sum() == 1.0 and R.impulse(4, 5, 3, 1)[3, 1] == 1.0
    assert len(set(R.impulse_sites(8, 8))) == 9 and len(set(R.impulse_sites(16, 12))) == 9
    gt = R.gt_mask(3, 5, 1027)
    assert (gt[:, 2, :] == -1).all() and (gt[:, :, -1] == -1).all() and {0.0, 1.0, 0.5, -1.0} == set(np.unique(gt).tolist())
    assert 0.4 < (gt == -1).mean() < 0.7


def test_case_tables_name_the_kernel_paths():
    """each store path and the multi-block x loop of postprocess_kernel has a named case, with and without a second resize"""
    ows = {(c[4][1], tuple(c[3]) == tuple(c[4])) for c in R.POST_CASES}
    assert any(ow % 4 == 0 and ow <= 1024 for ow, _ in ows) and any(ow % 4 and ow <= 1024 for ow, _ in ows)
    assert any(ow % 4 == 0 and ow > 1024 for ow, _ in ows) and any(ow % 4 and ow > 1024 for ow, _ in ows) and any(ow > 2048 for ow, _ in ows)
    assert {k for c in R.POST_CASES for k in [c[4][1]] if c[4][0] == 2} == set(range(1, 10))
    for ident in (True, False):
        assert any(ow % 4 == 0 for ow, i in ows if i == ident) and any(ow % 4 for ow, i in ows if i == ident)
    assert all(c[4][0] * c[4][1] * R.N_IMAGES < 100_000 for c in R.POST_CASES)
