"""The two activation-staging forms of the packed batch-1 decode GEMV (gemv1_p12m_kernel, hook ivlm_gemv1_bf12m_staging): form 1 -
every wave stages the K range its own MFMA steps read, loaded ahead of the first weight loads, block barrier behind the K loop -
against form 0 - the block stages the row cooperatively in front of a barrier.  What can go wrong is the K range a wave owns (uneven
and empty ranges, patches that read columns another wave staged, heads of the attention partials that straddle waves) and the order
of the RMS prologue's sum of squares, so the shapes are small and the comparison between the forms is bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

TOL = 3e-6  # of the output range, against fp64: the bound of test_gemv_bf12_is_lossless_and_equals_the_bf16_gemv for this kernel

# (N, K, act, rms, residual, patches planted in every step pair)
SHAPES = [
    (16, 64, "none", False, False, False),      # one step pair: every wave but the first is empty
    (32, 320, "none", False, False, False),     # five step pairs
    (48, 704, "none", False, False, False),     # eleven: 8 waves - 2, 2, 2, 2, 2, 1, none, none; 16 waves - five empty waves
    (48, 704, "none", False, False, True),
    (48, 1024, "swiglu", True, False, False),
    (64, 4096, "none", True, False, False),
    (32, 11008, "none", False, True, False),    # the 7B / 13B down_proj rows: uneven ranges, the last wave has 7 resp. 6 step pairs
    (32, 11008, "none", False, True, True),
    (32, 13824, "none", False, True, False),
]
PLANT_ROWS = (2, 21)  # two rows of different 16-row blocks: their patches belong to different waves


def _both_forms(lib, call):
    """call() under staging form 0, then twice under form 1 (the default, restored)."""
    try:
        assert lib.ivlm_gemv1_bf12m_staging(0) == 0
        y0 = call()
        assert lib.ivlm_gemv1_bf12m_staging(1) == 0
        y1, y1b = call(), call()
    finally:
        lib.ivlm_gemv1_bf12m_staging(1)
    return y0, y1, y1b


def _check(y0, y1, y1b, ref, what):
    import torch

    scale = float(ref.abs().max())
    err = float((y1.double().cpu() - ref).abs().max()) / scale
    print(f"\n[bf12 staging {what}] form 1 vs fp64: {err:.2e} of range; equal to form 0: {torch.equal(y1, y0)}")
    assert y1.shape == ref.shape and bool(torch.isfinite(y1).all())
    assert torch.equal(y1, y0), what   # (a) the same bits as the block-cooperative form
    assert err < TOL, (what, err)      # (b)
    assert torch.equal(y1, y1b), what  # (c)


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("N,K,act,rms,res,plant", SHAPES)
def test_per_wave_staging_equals_block_staging(hip_lib, cuda, N, K, act, rms, res, plant, waves):
    import torch

    from interactvlm_amd import ops

    nsp = K // 64
    g = torch.Generator().manual_seed(3 * N + K + plant)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    x = torch.randn(1, K, generator=g) * 2.0
    planted = 0
    if plant:  # in two rows one weight of EVERY step pair lies under the row's exponent window: the patch row of a wave reads
        for r in PLANT_ROWS:  # columns that every other wave staged
            w[r, 1] = 1.0  # (an O(1) entry: the window ends at 2^-14)
            for sp in range(nsp):
                col = sp * 64 + 8 + (3 * sp + r) % 48
                w[r, col] = 2e-7 if sp % 2 == 0 else 1e-30
                x[0, col] = 8.0 if sp % 4 == 0 else -8.0  # (so that the 2e-7 patches show in the low bits of the row's result)
                planted += 1
    w, x = w.to(cuda), x.to(cuda)
    gam = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().to(cuda) if rms else None
    r_ = torch.randn(1, N, generator=g).to(cuda) if res else None
    wp = ops.PackedBf12(w)
    assert wp.frag and wp.n_patches >= planted
    xd = x.double().cpu()
    if rms:
        xd = xd * torch.rsqrt((xd * xd).mean() + 1e-5) * gam.double().cpu()
    ref = xd @ w.double().cpu().t()
    if act == "swiglu":
        ref = torch.nn.functional.silu(ref[:, 0::2]) * ref[:, 1::2]
    if res:
        ref = ref + r_.double().cpu()
    try:
        if waves == 8:
            hip_lib.ivlm_gemv1_bf12m_tuning(0)  # no grid is "at most 0 blocks": the 8-wave form
        y0, y1, y1b = _both_forms(hip_lib, lambda: ops.linear_bf12(x, wp, act=act, residual=r_, rms=(gam, 1e-5) if rms else None))
    finally:
        hip_lib.ivlm_gemv1_bf12m_tuning(256)
    _check(y0, y1, y1b, ref, f"{N}x{K} {act} rms={rms} {waves} waves, {wp.n_patches} patches")


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("S", [4, 2])
@pytest.mark.parametrize("H,D", [(4, 128), (5, 128)])  # K = 512; K = 640: ten step pairs, a wave's range is half a head
def test_per_wave_staging_merges_the_attention_partials(hip_lib, cuda, H, D, S, waves):
    """The o_proj form: x[h][d] = sum_s e^(m_s - M) o_s[d] / sum_s e^(m_s - M) l_s merged from partials [H][S][D + 4] while the row
    is staged, with range maxima far apart."""
    import torch

    from interactvlm_amd import ops

    N, K = 32, H * D
    g = torch.Generator().manual_seed(H + 10 * S)
    ms = [-30.0, 0.0, 5.0, 40.0]
    parts = torch.zeros(H, 4, D + 4)  # (ops.linear_bf12 asks for room for four ranges; S of them are laid out [H][S][D + 4])
    o = torch.randn(H, S, D, generator=g)
    m = torch.tensor([[ms[(s + h) % 4] for s in range(S)] for h in range(H)])
    l = 0.5 + torch.rand(H, S, generator=g) * 50.0
    used = parts.view(-1)[: H * S * (D + 4)].view(H, S, D + 4)
    used[:, :, :D], used[:, :, D], used[:, :, D + 1] = o, m, l
    wgt = torch.exp(m.double() - m.double().max(dim=1, keepdim=True).values)  # [H][S]
    xd = ((wgt[:, :, None] * o.double()).sum(1) / (wgt * l.double()).sum(1, keepdim=True)).reshape(1, K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    res = torch.randn(1, N, generator=g)
    ref = xd @ w.double().t() + res.double()
    parts, w, res = parts.to(cuda), w.to(cuda), res.to(cuda)
    wp = ops.PackedBf12(w)
    assert wp.frag
    try:
        assert hip_lib.ivlm_decode_parts_tuning(S) == 0
        if waves == 8:
            hip_lib.ivlm_gemv1_bf12m_tuning(0)
        y0, y1, y1b = _both_forms(hip_lib, lambda: ops.linear_bf12(None, wp, residual=res, parts=(parts, D)))
    finally:
        hip_lib.ivlm_gemv1_bf12m_tuning(256)
        hip_lib.ivlm_decode_parts_tuning(4)
    _check(y0, y1, y1b, ref, f"partials H={H} D={D} S={S}, {waves} waves")


def test_staging_hook_rejects_other_forms(hip_lib, cuda):
    try:
        assert hip_lib.ivlm_gemv1_bf12m_staging(2) != 0 and hip_lib.ivlm_gemv1_bf12m_staging(-1) != 0
    finally:
        assert hip_lib.ivlm_gemv1_bf12m_staging(1) == 0
