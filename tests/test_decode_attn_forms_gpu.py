"""Every form of the single-query decode attention against ONE independent reference: torch fp64 on the CPU, built from the cache as
stored plus the exact new row (the construction of test_decode_attn_batch_equals_per_sequence).  The kernels share one body
(decode_attn.h: decode_attn_range), so the tests that compare them with each other no longer check it; these do, beyond the first
384-key tile of the one-block kernels and for ranges that start mid-slab and span several 96-key tiles of the split-KV ones."""
import functools

import pytest

pytestmark = pytest.mark.gpu

H, TMAX = 3, 1024
POS = (0, 1, 15, 16, 383, 384, 385, 800)
# fp32 evaluation of these inputs stays below 2e-6 of the fp64 reference (checked on the CPU), which leaves the bound of the existing
# tests of this arithmetic an order of magnitude for __expf
BOUND = 2e-5
# bf16 I/O (q, the new k and P rounded to bf16, a bf16 output row): the largest error of the build BEFORE the kernels shared a body, at
# positions 384 and 800 with D = 16 and 128, was PARENT_BF16IO_ERR (MI355X; D = 16: 3.858e-4 at 384, 3.855e-4 at 800; D = 128: 4.808e-4
# and 4.824e-4; one-block and batched forms alike); the bound is twice that
PARENT_BF16IO_ERR = 4.824e-4
BF16IO_BOUND = 2 * PARENT_BF16IO_ERR


def _rope(x, cos, sin, p, D):
    import torch

    c, s = torch.cat([cos[p], cos[p]]), torch.cat([sin[p], sin[p]])
    return x * c + torch.cat([-x[..., D // 2:], x[..., : D // 2]], -1) * s


def _reference(x, Kh, Vh, cos, sin, p, D, bf16_io=False):
    """x fp64 [3, H, D] (q | k | v of the new token), Kh / Vh fp64 [Tmax, H, D] the cache as stored -> (o [H*D], new k row, new v row)"""
    import torch

    qr, kr = _rope(x[0], cos, sin, p, D), _rope(x[1], cos, sin, p, D)
    kn = kr
    if bf16_io:  # the roundings the kernel documents for bf16 qkv: q and the new k after RoPE, the softmax weights before P.V
        qr, kn = qr.to(torch.bfloat16).double(), kr.to(torch.bfloat16).double()
    K_ = torch.cat([Kh[:p], kn[None]], 0)  # [p + 1, H, D]: history + the new row
    V_ = torch.cat([Vh[:p], x[2][None]], 0)
    a = torch.softmax(torch.einsum("hd,thd->ht", qr, K_) * D ** -0.5, -1)
    if bf16_io:
        a = a.to(torch.bfloat16).double()
    return torch.einsum("ht,thd->hd", a, V_).reshape(-1), kr, x[2]


@functools.lru_cache(maxsize=None)
def _case(D, cache, cuda):
    """Seeded inputs and their fp64 references, made once per (D, cache form) and shared, unchanged, by the tests: cache = "bf16" | "f16"
    (one plane of that type), "lo" (hi + lo bf16 planes) or "bf16io" (bf16 cache and bf16 qkv)."""
    import torch

    from interactvlm_amd import ops

    g = torch.Generator().manual_seed(41 + D)
    k32, v32 = torch.randn(TMAX, H, D, generator=g), torch.randn(TMAX, H, D, generator=g)
    q = torch.randn(len(POS), 3 * H * D, generator=g)
    dt = torch.float16 if cache == "f16" else torch.bfloat16
    planes = [k32.to(dt), v32.to(dt)]
    Kh, Vh = planes[0].double(), planes[1].double()
    if cache == "lo":
        planes += [(k32 - planes[0].float()).to(dt), (v32 - planes[1].float()).to(dt)]
        Kh, Vh = Kh + planes[2].double(), Vh + planes[3].double()
    if cache == "bf16io":
        q = q.to(torch.bfloat16)
    tab = ops.rope_table(TMAX, D, 10000.0, cuda)
    cos, sin = tab[0].double().cpu(), tab[1].double().cpu()
    refs = {p: _reference(q[i].double().view(3, H, D), Kh, Vh, cos, sin, p, D, cache == "bf16io") for i, p in enumerate(POS)}
    return {"q": q.to(cuda), "planes": [t.to(cuda) for t in planes], "tab": tab, "refs": refs, "dt": dt}


def _check_appended(kc, vc, p, ref, dt, what):
    """the appended rows are the rounded reference rows: equal, or within 2^-7 relative (an fp32 RoPE that lands across a rounding tie)"""
    import torch

    _, kr, vr = ref
    for got, want in ((kc[p], kr), (vc[p], vr)):
        assert torch.equal(got.cpu(), want.to(dt)) or \
            float((got.double().cpu() - want).abs().max()) < 2.0 ** -7 * float(want.abs().max()), what


def _err(got, ref, what):
    e = float((got.double().cpu().reshape(-1) - ref[0]).abs().max())
    print(f"{what}: max |err| {e:.3e}")
    return e


@pytest.mark.parametrize("cache", ["bf16", "f16"])
@pytest.mark.parametrize("D", [16, 128])
def test_one_block_and_batched_forms_beyond_the_first_tile(hip_lib, cuda, D, cache):
    """fp32 I/O, one-block kernel at every position of POS (first tile, its edge at 384, three tiles) and the batched kernel on the same
    inputs, B = 3 with one sequence at pos == Tmax (a zero row, its slab untouched): within 2e-5 of fp64, rows appended as rounded."""
    import torch

    from interactvlm_amd import ops

    c = _case(D, cache, cuda)
    k0, v0 = c["planes"]
    for i, p in enumerate(POS):
        kc, vc = k0.clone(), v0.clone()
        p_arg = torch.tensor([p], dtype=torch.int32, device=cuda) if p % 2 else p
        got = ops.llama_decode_attn(c["q"][i: i + 1].contiguous(), kc, vc, H, D, p_arg, 10000.0, D ** -0.5, table=c["tab"])
        assert _err(got, c["refs"][p], f"one-block D={D} {cache} pos={p}") < BOUND, p
        _check_appended(kc, vc, p, c["refs"][p], c["dt"], p)
        kc[p], vc[p] = k0[p], v0[p]
        assert torch.equal(kc, k0) and torch.equal(vc, v0), p  # nothing else was written
    for i in range(4):
        rows = [i, i + 4, 0]
        pos = [POS[i], POS[i + 4], TMAX]
        kc, vc = (torch.stack([t, t, t]).contiguous() for t in (k0, v0))
        got = ops.llama_decode_attn_batch(c["q"][rows].contiguous(), kc, vc, H, D, torch.tensor(pos, dtype=torch.int32, device=cuda),
                                          10000.0, D ** -0.5, table=c["tab"])
        assert float(got[2].abs().max()) == 0.0 and torch.equal(kc[2], k0) and torch.equal(vc[2], v0)
        for b in range(2):
            assert _err(got[b], c["refs"][pos[b]], f"batched D={D} {cache} pos={pos[b]}") < BOUND, pos
            _check_appended(kc[b], vc[b], pos[b], c["refs"][pos[b]], c["dt"], pos)


@pytest.mark.parametrize("D", [16, 128])
def test_hi_lo_planes_beyond_the_first_tile(hip_lib, cuda, D):
    """The "parity" cache form (K / V as hi + lo bf16 planes) at positions 383, 384 and 800, one-block and batched, against fp64 on
    hi + lo: the 2e-5 bound of test_rope_split_cache_and_decode_attention; the new row is appended unrounded (hi + lo to 1e-4)."""
    import torch

    from interactvlm_amd import ops

    c = _case(D, "lo", cuda)
    idx = [POS.index(p) for p in (383, 384, 800)]
    for i in idx:
        p = POS[i]
        kc, vc, kl, vl = (t.clone() for t in c["planes"])
        got = ops.llama_decode_attn(c["q"][i: i + 1].contiguous(), kc, vc, H, D, p, 10000.0, D ** -0.5, table=c["tab"], lo=(kl, vl))
        assert _err(got, c["refs"][p], f"one-block hi+lo D={D} pos={p}") < BOUND, p
        for hi, lo, want in ((kc, kl, c["refs"][p][1]), (vc, vl, c["refs"][p][2])):
            assert float(((hi[p].double() + lo[p].double()).cpu() - want).abs().max()) < 1e-4, p
    bc = [torch.stack([t, t, t]).contiguous() for t in c["planes"]]
    pos = [POS[i] for i in idx]
    got = ops.llama_decode_attn_batch(c["q"][idx].contiguous(), bc[0], bc[1], H, D, torch.tensor(pos, dtype=torch.int32, device=cuda),
                                      10000.0, D ** -0.5, table=c["tab"], lo=(bc[2], bc[3]))
    for b, p in enumerate(pos):
        assert _err(got[b], c["refs"][p], f"batched hi+lo D={D} pos={p}") < BOUND, p


@pytest.mark.parametrize("D", [16, 128])
def test_bf16_io_form_beyond_the_first_tile(hip_lib, cuda, D):
    """bf16 qkv / o at positions 384 and 800, one-block and batched, against the fp64 reference with q, the new k and P rounded to
    bf16 as the kernel documents.  The bound is not derived from the formats (the output row itself is rounded to bf16, and a
    rounding of P that lands on the other side of a tie moves a weight by a bf16 ulp): it is twice the error measured on the
    build before the kernels shared their body - see PARENT_BF16IO_ERR above."""
    import torch

    from interactvlm_amd import ops

    c = _case(D, "bf16io", cuda)
    idx = [POS.index(p) for p in (384, 800)]
    k0, v0 = c["planes"]
    errs = []
    for i in idx:
        p = POS[i]
        kc, vc = k0.clone(), v0.clone()
        got = ops.llama_decode_attn(c["q"][i: i + 1].contiguous(), kc, vc, H, D, p, 10000.0, D ** -0.5, table=c["tab"])
        assert got.dtype == torch.bfloat16
        errs.append(_err(got, c["refs"][p], f"one-block bf16 io D={D} pos={p}"))
        _check_appended(kc, vc, p, c["refs"][p], c["dt"], p)
    pos = [POS[i] for i in idx]
    kc, vc = (torch.stack([t, t]).contiguous() for t in (k0, v0))
    got = ops.llama_decode_attn_batch(c["q"][idx].contiguous(), kc, vc, H, D, torch.tensor(pos, dtype=torch.int32, device=cuda), 10000.0,
                                      D ** -0.5, table=c["tab"])
    errs += [_err(got[b], c["refs"][p], f"batched bf16 io D={D} pos={p}") for b, p in enumerate(pos)]
    assert max(errs) < BF16IO_BOUND, errs


@pytest.mark.parametrize("cache", ["bf16", "f16"])
@pytest.mark.parametrize("D", [16, 128])
def test_splitkv_and_parts_ranges_that_start_mid_slab(hip_lib, cuda, D, cache):
    """Position 800 cut into S = 3 ranges of 272 keys and S = 4 ranges of 208 (every range but the first starts mid-slab and spans
    three 96-key tiles): the split-KV kernel (merged by the last block) for both S and the parts form (S = 4; merged here in fp64 from
    the published (o, max, sum)) against the fp64 reference - not against the one-block kernel - within 2e-5."""
    import torch

    from interactvlm_amd import ops

    c = _case(D, cache, cuda)
    p, i = 800, POS.index(800)
    ref = c["refs"][p]
    q = c["q"][i: i + 1].contiguous()
    k0, v0 = c["planes"]
    scratch = ops.decode_attn_scratch(H, D, cuda)
    try:
        for S in (3, 4):
            assert hip_lib.ivlm_llama_decode_attn_splits(S) == 0
            kc, vc = k0.clone(), v0.clone()
            got = ops.llama_decode_attn(q, kc, vc, H, D, p, 10000.0, D ** -0.5, table=c["tab"], scratch=scratch)
            assert _err(got, ref, f"split-KV S={S} D={D} {cache} pos={p}") < BOUND, S
            _check_appended(kc, vc, p, ref, c["dt"], S)
    finally:
        hip_lib.ivlm_llama_decode_attn_splits(8)
    S = 4
    parts = torch.zeros(H * S * (D + 4), dtype=torch.float32, device=cuda)
    kc, vc = k0.clone(), v0.clone()
    ops.llama_decode_attn_parts(q, kc, vc, H, D, p, 10000.0, D ** -0.5, parts, table=c["tab"])
    pr = parts.double().cpu().view(H, S, D + 4)
    o, m, l = pr[..., :D], pr[..., D], pr[..., D + 1]
    assert bool((l > 0).all())  # 801 keys in ranges of 208: none is empty
    w = torch.exp(m - m.max(1, keepdim=True).values)  # [H, S]
    got = ((w[..., None] * o).sum(1) / (w * l).sum(1, keepdim=True)).reshape(-1)
    assert _err(got, ref, f"parts S={S} D={D} {cache} pos={p}") < BOUND
    _check_appended(kc, vc, p, ref, c["dt"], "parts")
