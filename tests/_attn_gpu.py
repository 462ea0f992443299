"""GPU-side helpers shared by the attention tests (test_attention_edges_gpu.py, test_attention_routes_gpu.py,
test_attention_f32_gpu.py): every tensor a kernel reads is a view into a larger buffer of finite poison (a neighbouring "head" of
poison directly behind each head's D columns, slack rows behind the last row), the output goes into a sentinel-filled buffer that
must be untouched outside the logical region."""
import torch

import _attn_ref as R

BF, F16 = torch.bfloat16, torch.float16
POISON, SENTINEL = 30720.0, 12288.0  # finite and exact in both types (an over-read shows as a wrong number, never as a fault)
SLACK = 4
MODES = [(BF, 0), (BF, 1), (F16, 0)]  # operand type, block shape (0: 4 waves / 128 queries, 1: 8-wave ping-pong / 256; fp16: 4 waves)
_mid = lambda m: f"{'bf16' if m[0] == BF else 'f16'}-{'pingpong' if m[1] else '4wave'}"
_id = lambda v: str(v).replace(" ", "")


class block_shape:
    def __init__(self, pp):
        from interactvlm_amd import _lib

        self.lib, self.pp = _lib.load(), pp

    def __enter__(self):
        self.lib.ivlm_attention_pingpong(self.pp)

    def __exit__(self, *exc):
        self.lib.ivlm_attention_pingpong(-1)


def _packed(x, rt, dev, ghost=None, pad=2):
    """x [B,H,S,D] -> the same values as a [B,H,S,D] view of a poisoned [B, S + SLACK, H, pad, D] buffer on the device: a head's D
    columns are followed by (pad - 1) * D columns of poison, the last row by SLACK rows of it (ghost [D]: the first slack row of every
    head).  Head stride pad * D, row stride H * pad * D: another pad, other strides."""
    B, H, S, D = x.shape
    buf = torch.full((B, S + SLACK, H, pad, D), POISON, dtype=rt)
    buf[:, 1::2] *= -1
    buf[:, :S, :, 0] = x.permute(0, 2, 1, 3).to(rt)
    if ghost is not None:
        buf[:, S, :, 0] = ghost.to(rt)
    return buf.to(dev)[:, :S, :, 0].permute(0, 2, 1, 3)


def _out_buffer(B, H, Sq, D, rt, dev):
    buf = torch.full((B, Sq + SLACK, H, 2, D), SENTINEL, dtype=rt, device=dev)
    return buf, buf[:, :Sq, :, 0].permute(0, 2, 1, 3)


def _assert_untouched(buf, Sq):
    rest = buf.clone()
    rest[:, :Sq, :, 0] = SENTINEL
    assert bool((rest == SENTINEL).all()), "the kernel wrote outside the logical [B, Sq, H, D] region of its output"


def _attend(q, k, v, rt, dev, scale, ghost=(None, None), **kw):
    """ops.attention on poisoned-buffer views of q [B,H,Sq,D], k / v [Bk,H,Sk,D] (cpu), out= a sentinel buffer; -> cpu [B,H,Sq,D]."""
    from interactvlm_amd import ops

    B, H, Sq, D = q.shape
    qd, kd, vd = _packed(q, rt, dev), _packed(k, rt, dev, ghost[0]), _packed(v, rt, dev, ghost[1])
    if kw.get("q_lo") is True:
        kw["q_lo"] = _packed(torch.zeros_like(q), rt, dev)
    buf, out = _out_buffer(B, H, Sq, D, rt, dev)
    got = ops.attention(qd, kd, vd, scale, out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and got.dtype == rt
    _assert_untouched(buf, Sq)
    return out.cpu()


def _attend_f32(q, k, v, dev, scale, ghost=(None, None), k_pad=2, v_pad=3, kv_batches=None):
    """ops.attention_f32 on poisoned-buffer views of fp32 q [B,H,Sq,D], k / v [Bk,H,Sk,D] (cpu), out= a sentinel buffer; -> cpu
    [B,H,Sq,D].  k and v sit in buffers of DIFFERENT padding: k_rs != v_rs and k_hs != v_hs (all strides stay multiples of 4 floats,
    all bases 16-byte aligned).  kv_batches = n: the call gets the first n batches of k / v, the others lie behind them in the same
    buffers (what a kernel with a wrong K/V batch index then reads is another batch's rows, not unmapped memory)."""
    from interactvlm_amd import ops

    F32 = torch.float32
    B, H, Sq, D = q.shape
    qd, kd, vd = _packed(q, F32, dev), _packed(k, F32, dev, ghost[0], pad=k_pad), _packed(v, F32, dev, ghost[1], pad=v_pad)
    assert kd.stride(2) != vd.stride(2) and kd.stride(1) != vd.stride(1)
    assert all(s % 4 == 0 for t in (qd, kd, vd) for s in t.stride()[:3]) and all(t.data_ptr() % 16 == 0 for t in (qd, kd, vd))
    if kv_batches is not None:
        kd, vd = kd[:kv_batches], vd[:kv_batches]
    buf, out = _out_buffer(B, H, Sq, D, F32, dev)
    got = ops.attention_f32(qd, kd, vd, scale, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == F32
    _assert_untouched(buf, Sq)
    return out.cpu()


def _attend_split(q, k, v, dev, scale, ghost=(None, None), **kw):
    """ops.attention_split with zero lo planes (the probe values are exact in bf16: the remainders ARE zero); the output a
    [B, Sq, 2, H, D] region inside a sentinel-filled flat buffer; -> hi + lo as fp64 [B,H,Sq,D]."""
    from interactvlm_amd import ops

    B, H, Sq, D = q.shape
    planes = []
    for t, gh in ((q, None), (k, ghost[0]), (v, ghost[1])):
        planes += [_packed(t, BF, dev, gh), _packed(torch.zeros_like(t), BF, dev)]
    n, pad = B * Sq * 2 * H * D, 4 * 2 * H * D
    flat = torch.full((n + 2 * pad,), SENTINEL, dtype=BF, device=dev)
    out = flat[pad: pad + n].view(B, Sq, 2, H, D)
    ops.attention_split(*planes, scale, out=out, **kw)
    assert bool((flat[:pad] == SENTINEL).all()) and bool((flat[pad + n:] == SENTINEL).all()), "split output overrun"
    o = out.cpu().double()
    return (o[:, :, 0] + o[:, :, 1]).permute(0, 2, 1, 3)


def _bh(t, B, H, rt=None):
    t = t[None, None].expand(B, H, *t.shape)
    return t if rt is None else t.to(rt)


def _assert_margin(got, o, wabs, emu, rt, what):
    gs = R.ratio_stats(got, o, wabs, rt)
    print(f"\n[{what}] ratio max {gs[0]:.3f} rms {gs[1]:.3f}  (emulation: max {emu[0]:.3f} rms {emu[1]:.3f})")
    assert gs[0] <= R.MAX_MARGIN * emu[0], f"{what}: max ratio {gs[0]:.3f} > {R.MAX_MARGIN} x {emu[0]:.3f}"
    assert gs[1] <= R.RMS_MARGIN * emu[1], f"{what}: rms ratio {gs[1]:.3f} > {R.RMS_MARGIN} x {emu[1]:.3f}"


def _cat_table(tab_h, tab_w, dev):
    n = tab_h.shape[0] + tab_w.shape[0]
    cat = torch.zeros((n + 63) // 64 * 64, tab_h.shape[1], dtype=tab_h.dtype)
    cat[: tab_h.shape[0]] = tab_h
    cat[tab_h.shape[0]: n] = tab_w
    return cat.to(dev)
