"""The mask-resampling kernels against a float64 reference, at arbitrary photo sizes and at the edges.

Kernels: ``postprocess_kernel`` (ivlm_postprocess_masks, ivlm_postprocess_masks_valid), ``lift_plan_lowres_kernel``
(ivlm_lift_mesh_plan_lowres) and ``resize_bilinear_kernel`` (ivlm_resize_bilinear), which share csrc/bilinear.h.  The reference
(``post64`` / ``resize64``), the bound and the case tables are in tests/_resample_ref.py; tests/test_resample_ref_cpu.py shows that the
bound admits a correct fp32 evaluation and misses a one-pixel shift by more than 100 x.  Every comparison is per pixel against
``bound``, which is derived from the input (no flat tolerance but the 1e-6 of the sigmoid and the 1e-3 of the lift, both from
tests/test_lift_gpu.py).  Outputs of the C entry points lie between guard words that must keep their bits.

Worst err / bound measured on an MI355X (every test prints its own figure; fp32 low-res | bf16 low-res):
  postprocess_kernel, raw logits        0.120 | 0.100   (ramp, 8x8 -> 32x21 -> 47x31)
  postprocess_kernel, sigmoid           0.050 | 0.044   (smooth, 1x1 -> 5x6 | 256x256 -> 1024x683 -> 7x1367)
  postprocess_kernel, impulse probes    0.045 | 0.045   (8x8 -> 32x21 -> 47x31)
  postprocess_kernel, sigmoid under gt  0.075 | 0.061   (8x8 -> 32x21 -> 47x31)
  resize_bilinear_kernel, fp32 output   0.132           (ramp, 16x12 -> 5x1027); bf16 output: every stored value inside its window
  lift_plan_lowres_kernel               bit-equal to the two-step path
The kernels use about an eighth of the bound.  The bound stays as derived: it is a worst case over roundings that these inputs do
not all meet, and a one-tap error misses it by a factor of 100 to 10^6 (tests/test_resample_ref_cpu.py).
"""
import numpy as np
import pytest
import torch

import _resample_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 4  # IVLM_F32, IVLM_BF16, IVLM_F16
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dev, bf16=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)
    return t.to(torch.bfloat16) if bf16 else t  # (exact where the values are bf16 values already)


def _guarded(numel, dev):
    """-> (buffer of GUARD + numel + GUARD int32 guard words, float32 view of the numel results)"""
    buf = torch.full((numel + 2 * R.GUARD,), R.GUARD_BITS, dtype=torch.int32, device=dev)
    return buf, buf[R.GUARD: R.GUARD + numel].view(torch.float32)


def _guards_intact(buf):
    g = torch.cat([buf[: R.GUARD], buf[-R.GUARD:]])
    return bool((g == R.GUARD_BITS).all())


def _postprocess(lib, dev, low_t, case, sigmoid=0, gt=None, ignore=-1.0):
    """one launch through the C entry point into a fresh guarded buffer -> float32 [n, oh, ow] (still on the device)"""
    h, w, img, ins, orig = case
    n = low_t.shape[0]
    assert tuple(low_t.shape) == (n, h, w) and low_t.is_contiguous()
    buf, out = _guarded(n * orig[0] * orig[1], dev)
    dt = BF16 if low_t.dtype == torch.bfloat16 else F32
    if gt is None:
        rc = lib.ivlm_postprocess_masks(low_t.data_ptr(), dt, n, h, w, img, ins[0], ins[1], orig[0], orig[1], sigmoid, out.data_ptr(), _stream())
    else:
        assert gt.numel() == out.numel() and gt.dtype == torch.float32 and gt.is_contiguous()
        rc = lib.ivlm_postprocess_masks_valid(low_t.data_ptr(), dt, n, h, w, img, ins[0], ins[1], orig[0], orig[1], gt.data_ptr(), ignore,
                                              out.data_ptr(), _stream())
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert _guards_intact(buf), "guard words around the output were written"
    return out.view(n, orig[0], orig[1])


def _report(what, err, e):
    ratio = R.worst(err, e)
    print(f"[resample] {what}: worst err / bound = {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("kind", ("smooth", "ramp"))
@pytest.mark.parametrize("case", R.POST_CASES, ids=R.case_id)
def test_postprocess_within_bound(hip_lib, cuda, case, kind, bf16):
    low, ref, e, e_sig = R.post_reference(case, kind, bf16)
    low_t = _dev(low, cuda, bf16)
    for sigmoid in (0, 1):
        got_t = _postprocess(hip_lib, cuda, low_t, case, sigmoid)
        assert torch.equal(got_t, _postprocess(hip_lib, cuda, low_t, case, sigmoid)), "a second launch gives other bits"
        got = got_t.cpu().numpy().astype(np.float64)
        exp, tol = (R.sigmoid64(ref), e_sig) if sigmoid else (ref, e)
        ratio = _report(f"postprocess{'_sigmoid' if sigmoid else ''} {'bf16' if bf16 else 'f32'} {kind} {R.case_id(case)}", np.abs(got - exp), tol)
        assert ratio <= 1.0


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("case", R.IMPULSE_CASES, ids=R.case_id)
def test_postprocess_impulse_probes(hip_lib, cuda, case, bf16):
    """a single 1 at the corners, on the edges and inside: its support (zeros elsewhere) and the full weight of the clamped taps"""
    h, w, img, ins, orig = case
    low = np.stack([R.impulse(h, w, r, c) for r, c in R.impulse_sites(h, w)])
    ref, e = R.post64(low, img, ins, orig), R.bound(low, img, ins, orig)
    got = _postprocess(hip_lib, cuda, _dev(low, cuda, bf16), case).cpu().numpy().astype(np.float64)
    assert _report(f"postprocess impulse {'bf16' if bf16 else 'f32'} {R.case_id(case)}", np.abs(got - ref), e) <= 1.0
    assert ref.max() >= 0.5 and (ref == 0).mean() > 0.9  # (the probes are seen, and most of the output must be zero)
    # clamped taps at full weight: where an output pixel is the corner impulse itself, it is stored exactly
    whole = ref == 1.0
    assert np.array_equal(got[whole], ref[whole]) and (whole.any() or orig[0] < ins[0])


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("case", R.VALID_CASES, ids=R.case_id)
def test_postprocess_masks_valid(hip_lib, cuda, case, bf16):
    """sigmoid where gt != ignore_label, raw logits elsewhere"""
    low, ref, e, e_sig = R.post_reference(case, "smooth", bf16)
    low_t = _dev(low, cuda, bf16)
    n, (oh, ow) = low.shape[0], case[4]
    gt = R.gt_mask(n, oh, ow)
    keep = gt != -1.0
    got = _postprocess(hip_lib, cuda, low_t, case, gt=_dev(gt, cuda)).cpu().numpy().astype(np.float64)
    exp = np.where(keep, R.sigmoid64(ref), ref)
    tol = np.where(keep, np.broadcast_to(e_sig, ref.shape), np.broadcast_to(e, ref.shape))
    assert _report(f"postprocess_valid {'bf16' if bf16 else 'f32'} {R.case_id(case)}", np.abs(got - exp), tol) <= 1.0
    # gt nowhere / everywhere the ignore label: the bits of apply_sigmoid = 1 / 0
    nowhere = _postprocess(hip_lib, cuda, low_t, case, gt=_dev(np.where(keep, gt, 0.25), cuda))
    assert torch.equal(nowhere, _postprocess(hip_lib, cuda, low_t, case, 1))
    everywhere = _postprocess(hip_lib, cuda, low_t, case, gt=_dev(np.full_like(gt, -1.0), cuda))
    assert torch.equal(everywhere, _postprocess(hip_lib, cuda, low_t, case, 0))
    # another ignore label is honoured
    other = _postprocess(hip_lib, cuda, low_t, case, gt=_dev(gt, cuda), ignore=0.5).cpu().numpy().astype(np.float64)
    k2 = gt != 0.5
    assert R.worst(np.abs(other - np.where(k2, R.sigmoid64(ref), ref)), np.where(k2, np.broadcast_to(e_sig, ref.shape), np.broadcast_to(e, ref.shape))) <= 1.0


@pytest.mark.parametrize("kind", ("smooth", "ramp"))
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=R.case_id)
def test_resize_bilinear_f32(hip_lib, cuda, case, kind):
    from interactvlm_amd import ops

    (h, w), (oh, ow) = case
    src = R.make_input(kind, R.N_IMAGES, h, w)
    ref, e = R.resize64(src, oh, ow), R.bound(src)
    got = ops.resize_bilinear(_dev(src, cuda), (oh, ow))
    assert got.dtype == torch.float32 and tuple(got.shape) == (R.N_IMAGES, oh, ow)
    assert _report(f"resize_bilinear f32 {kind} {R.case_id(case)}", np.abs(got.cpu().numpy().astype(np.float64) - ref), e) <= 1.0


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=R.case_id)
def test_resize_bilinear_bf16(hip_lib, cuda, case):
    """the stored bf16 value lies in [bf16(ref - e), bf16(ref + e)] (rounding is monotonic); for all but at most 2 % of the pixels of
    this test that window is ONE value (tests/test_resample_ref_cpu.py)"""
    from interactvlm_amd import ops

    (h, w), (oh, ow) = case
    src = R.make_input("smooth24", R.N_IMAGES, h, w)
    lo, hi = R.bf16_window(R.resize64(src, oh, ow), R.bound(src))
    got = ops.resize_bilinear(_dev(src, cuda), (oh, ow), dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (R.N_IMAGES, oh, ow)
    g = got.float().cpu().numpy().astype(np.float64)
    bad = (g < lo) | (g > hi)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} stored values outside the window"


@pytest.mark.parametrize("case", R.LIFT_CASES, ids=R.case_id)
def test_fused_lowres_lift(hip_lib, cuda, case):
    """ivlm_lift_mesh_plan_lowres == ivlm_postprocess_masks -> ivlm_lift_mesh_plan bit for bit, at odd and multi-block sizes; mode 0
    within the 1e-3 of test_fused_lowres_lift_equals_two_step of the oracle's lift of post64's masks"""
    from interactvlm_amd import ops, synth
    from oracle import cref

    h, w, img, ins, (oh, ow) = case
    B, V, NV = R.N_IMAGES, 2, 50
    vid, bary = synth.synth_mesh_tables(V, oh, ow, NV, fg=0.4, seed=3, patch=3)
    plan = ops.LiftPlan(torch.from_numpy(vid).to(cuda).to(torch.int32), _dev(bary, cuda), NV)
    low = R.smooth(B * V, h, w)
    for bf16 in (False, True):
        lw = R.to_bf16(low) if bf16 else low
        low_t = _dev(lw, cuda, bf16)
        full = ops.postprocess_masks(low_t.view(B * V, 1, h, w), ins, (oh, ow), img_size=img).view(B, V, oh, ow)
        for mode, param in ((0, 20.0), (1, 0.3)):
            two = ops.lift_mesh_plan(full, plan, mode=mode, param=param)
            one = ops.lift_mesh_plan_lowres(low_t.view(B, V, h, w), plan, ins, (oh, ow), img, mode=mode, param=param)
            assert torch.equal(one, two), f"mode {mode}, {'bf16' if bf16 else 'f32'}"
            if mode == 0:
                masks = R.post64(lw, img, ins, (oh, ow)).reshape(B, V, oh, ow).astype(np.float32)
                exp, _ = cref.lift_mesh_soft(masks, vid, bary, NV)
                np.testing.assert_allclose(one.cpu().numpy(), exp, atol=1e-3, rtol=0)
                assert exp.max() - exp.min() > 0.2  # (the vertices differ by far more than the tolerance)


def test_host_rejections(hip_lib, cuda):
    """bad sizes and dtypes are refused on the host; the pointers are valid and nothing is launched"""
    lib = hip_lib
    low = torch.zeros(64, device=cuda)
    gt = torch.zeros(64, device=cuda)
    buf, out = _guarded(64, cuda)
    good = dict(dt=F32, n=1, h=4, w=4, img=8, in_h=8, in_w=8, oh=2, ow=2)

    def plain(**kw):
        a = dict(good, **kw)
        return lib.ivlm_postprocess_masks(low.data_ptr(), a["dt"], a["n"], a["h"], a["w"], a["img"], a["in_h"], a["in_w"], a["oh"], a["ow"], 0,
                                          out.data_ptr(), _stream())

    def valid(gtp=None, **kw):
        a = dict(good, **kw)
        return lib.ivlm_postprocess_masks_valid(low.data_ptr(), a["dt"], a["n"], a["h"], a["w"], a["img"], a["in_h"], a["in_w"], a["oh"], a["ow"],
                                                gt.data_ptr() if gtp is None else gtp, -1.0, out.data_ptr(), _stream())

    bad = [dict(in_h=9), dict(in_w=9), dict(oh=65536), dict(n=65536)] + [{k: 0} for k in ("n", "h", "w", "img", "in_h", "in_w", "oh", "ow")]
    for call in (plain, valid):
        for kw in bad:
            assert call(**kw) == ERR_INVALID_ARG, (call.__name__, kw)
        assert call(dt=F16) == ERR_UNSUPPORTED
    assert valid(gtp=0) == ERR_INVALID_ARG
    resize = lambda dt=F32, oh=2: lib.ivlm_resize_bilinear(low.data_ptr(), 1, 4, 4, out.data_ptr(), dt, oh, 2, _stream())
    assert resize(dt=F16) == ERR_UNSUPPORTED
    assert resize(oh=65536) == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((buf == R.GUARD_BITS).all()), "a rejected call wrote to its output"
    # ... and the same calls with good arguments are accepted
    assert plain() == OK and valid() == OK and resize() == OK
    torch.cuda.synchronize()
    assert _guards_intact(buf)
