"""The cases of tests/test_dense_bits_gpu.py and tests/golden/make_golden_dense_bits.py: one per distinct argument path of the dense,
data-movement and decode-attention wrappers of ``interactvlm_amd/ops.py``, at the smallest shapes that take the path.  A case is a
function of the device that calls public wrappers and returns a list of tensors; ``record`` turns it into strings that compare equal
exactly when every bit does.  These kernels sum in fixed orders, so a record made by one build holds every later one to the same
arguments at every C call: a wrapper that hands over another flag, stride, code or pointer changes an output bit here.

All inputs are seeded from ``synth``, so they are the same numbers wherever the cases run.  ``llama_attn_oproj`` is not here (its
kernel needs all of its blocks co-resident; test_graph_decode_with_fused_attn_oproj_matches_eager covers it).
"""
import hashlib

import torch

from interactvlm_amd import ops, synth

CASES = {}
BF16, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
_VIEW = {torch.float32: torch.int32, torch.int32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
         torch.uint8: torch.uint8}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def encode(t):
    """a tensor (fp32, int32, bf16, fp16 or uint8) -> the hex of its raw bytes; their sha256 when they are more than 64, so that the
    golden file stays small"""
    t = t.detach().cpu().contiguous()
    assert t.dtype in _VIEW, t.dtype
    raw = t.view(_VIEW[t.dtype]).numpy().tobytes()
    return raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


def record(name, dev):
    return [f"{tuple(t.shape)} {str(t.dtype)[6:]} {encode(t)}" for t in CASES[name](dev)]


def _n(dev, key, shape, std=1.0, dtype=F32):
    """N(0, std^2) values named by ``key`` as a device tensor of ``dtype``"""
    return torch.from_numpy(synth.synth_normal("dense_bits/" + key, shape, std)).to(dev).to(dtype)


def _i(dev, values):
    return torch.tensor(values, dtype=I32, device=dev)


# ---- linear: the tile GEMMs (M = 48, N = K = 128) ---------------------------------------------------------------------------------------
M, N, K = 48, 128, 128


def _xwb(dev, tag, m=M, n=N, k=K, dtype=BF16):
    return _n(dev, tag + "/x", (m, k), 1.0, dtype), _n(dev, tag + "/w", (n, k), 0.1, BF16), _n(dev, tag + "/b", (n,), 0.5, BF16)


@case
def linear_tile_plain(dev):
    x, w, b = _xwb(dev, "tile")
    return [ops.linear(x, w, b, act="gelu", residual=_n(dev, "tile/r", (M, N), 1.0, BF16))]


@case
def linear_tile_strided(dev):
    """x and out= column slices of wider buffers, an fp32 residual of 16 rows taken modulo, fp32 output"""
    _, w, b = _xwb(dev, "tile")
    xw = _n(dev, "strided/x", (M, K + 64), 1.0, BF16)
    ow = torch.zeros(M, N + 32, dtype=F32, device=dev)
    out = ops.linear(xw[:, 32: 32 + K], w, b, residual=_n(dev, "strided/r", (16, N)), res_mod=16, out=ow[:, 16: 16 + N], out_f32=True)
    return [out, ow]


@case
def linear_tile_swiglu(dev):
    x, w, b = _xwb(dev, "swiglu", n=256)
    return [ops.linear(x, w, b, act="swiglu")]


@case
def linear_tile_out_rows_a_rows(dev):
    """the gather prologue and the scatter epilogue: product row m reads x[a_rows[m]] and lands in row out_rows[m] (one row dropped)
    on top of that row's residual"""
    x, w, b = _xwb(dev, "tile")
    a_rows = _i(dev, [(5 * m + 3) % M for m in range(M)])
    out_rows = _i(dev, [-1 if m == 7 else (M - 1 - m) for m in range(M)])
    stream = _n(dev, "rows/stream", (M, N), 1.0, BF16)
    before = stream.clone()
    return [ops.linear(x, w, b, residual=stream, out=stream, out_rows=out_rows, a_rows=a_rows), before]


@case
def linear_tile_split(dev):
    x32 = _n(dev, "split/x", (M, K))
    _, w, b = _xwb(dev, "tile")
    xs = ops.split_rows(x32)
    return [xs, ops.linear(xs, w, b, act="gelu", a_split=True, out_split=True)]


@case
def linear_tile_f16(dev):
    """IEEE-half operands: fp16 out, and split fp16 operands into a split fp16 result (the rows layernorm(out_split, out_f16) makes)"""
    x, w, b = _xwb(dev, "f16", dtype=F16)
    w16 = ops.bf16_to_f16(w)
    lw, lb = _n(dev, "f16/lw", (K,), 1.0, BF16), _n(dev, "f16/lb", (K,), 0.1, BF16)
    xs = ops.layernorm(_n(dev, "f16/x32", (M, K)), lw, lb, 1e-6, out_split=True, out_f16=True)
    return [w16, ops.linear(x, w16, b, out_f16=True), ops.linear(xs, w16, b, a_split=True, out_split=True, out_f16=True)]


@case
def linear_tile_panel_weight(dev):
    x, w, b = _xwb(dev, "tile")
    wp = ops.panel_weight(w)
    return [wp, ops.linear(x, wp, b, act="gelu")]


# ---- linear: split-K (M = 40, N = 256, K = 1024: two slices) ---------------------------------------------------------------------------
def _splitk(dev, fused):
    m, n, k = 40, 256, 1024
    assert ops._splitk_choice(m, n, k, "none", None) == 2
    x, w, b = _xwb(dev, "splitk", m, n, k)
    was = ops.SPLITK_FUSED
    ops.SPLITK_FUSED = fused
    try:
        out = [ops.linear(x, w, b, residual=_n(dev, "splitk/r", (m, n)), out_f32=True)]
        if fused:
            out.append(ops._splitk_counters(x.device).sum().to(I32).reshape(1))
    finally:
        ops.SPLITK_FUSED = was
    return out


@case
def linear_splitk(dev):
    return _splitk(dev, False)


@case
def linear_splitk_fused(dev):
    return _splitk(dev, True)


# ---- linear: the weight-streaming kernels (M <= 16) ------------------------------------------------------------------------------------
@case
def linear_stream(dev):
    _, w, b = _xwb(dev, "stream", n=256, k=256)
    gam = _n(dev, "stream/gam", (256,), 1.0, BF16)
    x1 = _n(dev, "stream/x1", (1, 256))
    return [ops.linear(x1, w, b, act="silu", residual=_n(dev, "stream/r1", (1, 256)), out_f32=True, rms=(gam, 1e-5)),
            ops.linear(x1.to(BF16), w, b),
            ops.linear(_n(dev, "stream/x12", (12, 256)), w, b, out_f32=True)]


# ---- fp8 ---------------------------------------------------------------------------------------------------------------------------------
@case
def linear_fp8_kinds(dev):
    x, w, b = _xwb(dev, "fp8")
    xq, sa = ops.quantize_fp8(x)
    wq, sw = ops.quantize_fp8(w)
    so = torch.full((1,), 0.05, dtype=F32, device=dev)
    r = _n(dev, "fp8/r", (M, N))
    out = [xq, sa, wq, sw]
    out.append(ops.linear_fp8(xq, wq, sa, sw, b, act="gelu"))
    out.append(ops.linear_fp8(xq, wq, sa, sw, b, residual=r, out_kind="f32"))
    out.append(ops.linear_fp8(xq, wq, sa, sw, b, act="gelu", out_kind="fp8", scale_out=so))
    a_rows = _i(dev, [(7 * m + 1) % M for m in range(M)])
    out_rows = _i(dev, [-1 if m == 3 else (M - 1 - m) for m in range(M)])
    stream = r.to(BF16)
    out.append(ops.linear_fp8(xq, wq, sa, sw, b, residual=stream, out=stream, out_rows=out_rows, a_rows=a_rows))
    return out


@case
def linear_fp8w(dev):
    _, w, b = _xwb(dev, "fp8w", n=256, k=256)
    wq, sw = ops.quantize_fp8(w)
    x = _n(dev, "fp8w/x", (1, 256))
    gam = _n(dev, "fp8w/gam", (256,), 1.0, BF16)
    return [ops.linear_fp8w(x, wq, sw, b, residual=_n(dev, "fp8w/r", (1, 256)), rms=(gam, 1e-5)),
            ops.linear_fp8w(x, wq, sw, act="swiglu", out_f32=False)]


# ---- the 12-bit weights ------------------------------------------------------------------------------------------------------------------
def _planes(wp):
    return [wp.P, wp.E, wp.ebase, wp.patch_ptr, wp.patch_col, wp.patch_val, wp.unpack()]


def _bf12_weight(dev, rows=256):
    w = _n(dev, "bf12/w", (rows, 256), 0.05, BF16)
    w[3, 5], w[17, 200] = 1e-12, -3e-9  # nonzero weights below their rows' exponent windows: patches
    return w


@case
def bf12_pack_both_packers(dev):
    w = _bf12_weight(dev)
    return _planes(ops.PackedBf12(w, packer="c")) + _planes(ops.PackedBf12(w, packer="torch")) + _planes(ops.PackedBf12(w, fragments=False))


@case
def linear_bf12_forms(dev):
    w = _bf12_weight(dev)
    wp = ops.PackedBf12(w)
    b, gam = _n(dev, "bf12/b", (256,), 0.5, BF16), _n(dev, "bf12/gam", (256,), 1.0, BF16)
    x1, x4 = _n(dev, "bf12/x1", (1, 256)), _n(dev, "bf12/x4", (4, 256))
    out = [ops.linear_bf12(x1, wp, b, act="silu", residual=_n(dev, "bf12/r1", (1, 256)), rms=(gam, 1e-5)),
           ops.linear_bf12(x4, wp, b, residual=_n(dev, "bf12/r4", (4, 256), 1.0, BF16), out_f32=False),
           ops.linear_bf12(x1, ops.PackedBf12(w, fragments=False), b)]
    wpad = ops.PackedBf12(_bf12_weight(dev, 250), pad_rows=True)
    out += _planes(wpad) + [ops.linear_bf12(x1, wpad)]
    return out


@case
def linear_bf12_parts(dev):
    """the o_proj that merges the split-KV partials of llama_decode_attn_parts (H = 2, D = 128) while it stages its row"""
    H, D, Tmax, p = 2, 128, 1024, 800
    kc, vc = _n(dev, "parts/k", (Tmax, H, D), 1.0, BF16), _n(dev, "parts/v", (Tmax, H, D), 1.0, BF16)
    tab = ops.rope_table(Tmax, D, 10000.0, dev)
    parts = torch.zeros(H * 4 * (D + 4), dtype=F32, device=dev)
    ops.llama_decode_attn_parts(_n(dev, "parts/qkv", (1, 3 * H * D)), kc, vc, H, D, p, 10000.0, D ** -0.5, parts, table=tab)
    wp = ops.PackedBf12(_bf12_weight(dev))
    return [parts, kc[p], vc[p], ops.linear_bf12(None, wp, residual=_n(dev, "parts/r", (1, 256)), parts=(parts, D))]


# ---- norms -----------------------------------------------------------------------------------------------------------------------------
@case
def layernorm_kinds(dev):
    x = _n(dev, "ln/x", (5, 256))
    w, b = _n(dev, "ln/w", (256,), 1.0, BF16), _n(dev, "ln/b", (256,), 0.1, BF16)
    sc = torch.full((1,), 0.02, dtype=F32, device=dev)
    out = [ops.layernorm(x, w, b), ops.layernorm(x.to(BF16), w, b, 1e-6, gelu=True), ops.layernorm(x, w, b, out_f32=True),
           ops.layernorm(x, w, b, out_f16=True), ops.layernorm(x, w, b, out_split=True), ops.layernorm(x, w, b, out_split=True, out_f16=True),
           ops.layernorm(x, w, b, fp8_scale=sc)]
    buf = torch.zeros(8, 256, dtype=F32, device=dev)
    out.append(ops.layernorm(x, w, b, out=buf, out_rows=_i(dev, [6, 0, 3, 7, 1])))
    return out


@case
def rmsnorm_kinds(dev):
    x, w = _n(dev, "rms/x", (5, 256)), _n(dev, "rms/w", (256,), 1.0, BF16)
    sc = torch.full((1,), 0.02, dtype=F32, device=dev)
    return [ops.rmsnorm(x, w), ops.rmsnorm(x.to(BF16), w, 1e-6), ops.rmsnorm(x, w, out_f32=True), ops.rmsnorm(x, w, out_f16=True),
            ops.rmsnorm(x, w, out_split=True), ops.rmsnorm(x, w, fp8_scale=sc)]


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------
@case
def gather_rows_kinds(dev):
    src = _n(dev, "gather/src", (9, 64))
    idx = _i(dev, [4, -1, 8, 0, 4, 2, 7])
    addw = _n(dev, "gather/add", (7, 96), 1.0, BF16)
    sc = torch.full((1,), 0.03, dtype=F32, device=dev)
    return [ops.gather_rows(src, idx), ops.gather_rows(src.to(BF16), idx, out_kind="f32"), ops.gather_rows(src, idx, out_kind="bf16"),
            ops.gather_rows(src, idx, out_kind="split"), ops.gather_rows(src, idx, out_kind="fp8", scale=sc),
            ops.gather_rows(src, idx, add=addw[:, 16: 80]), ops.gather_rows(src.to(BF16))]


@case
def add_rows_forms(dev):
    a, b = _n(dev, "add/a", (7, 64)), _n(dev, "add/b", (3, 64), 1.0, BF16)
    return [ops.add_rows(a, b), ops.add_rows(a, b, op="mul"), ops.add_rows(a.to(BF16), b), ops.add_rows(a, b, out_kind="split"),
            ops.add_rows(a, b, out_kind="bf16")]


@case
def small_row_kernels(dev):
    """split_rows, fill_rows, amax, bf16_to_f16, argmax with and without bump"""
    x = _n(dev, "rows/x", (6, 64))
    buf = _n(dev, "rows/buf", (9, 96), 1.0, BF16)
    ops.fill_rows(buf[:, :64], _i(dev, [8, 2, 5]), _n(dev, "rows/row", (64,), 1.0, BF16))
    logits = _n(dev, "rows/logits", (3, 1000))
    bump = _i(dev, [10, 20, 30])
    return [ops.split_rows(x), buf, ops.amax(x), ops.amax(x.to(BF16)), ops.bf16_to_f16(x.to(BF16)), ops.argmax(logits),
            ops.argmax(logits, bump=bump), bump]


@case
def data_movement(dev):
    """the im2col kernels, dense_pe, resize_bilinear"""
    xs = ops.split_rows(_n(dev, "mv/xs", (2 * 5 * 7, 8)))
    gauss = _n(dev, "mv/gauss", (2, 16))
    src = _n(dev, "mv/src", (2, 3, 9, 7))
    return [ops.im2col_nchw(_n(dev, "mv/nchw", (2, 3, 28, 28), 1.0, BF16), 14, 14), ops.im2col3x3_nhwc(_n(dev, "mv/nhwc", (2, 5, 7, 8), 1.0, BF16)),
            xs, ops.im2col3x3_nhwc_split(xs, 2, 5, 7, 8), ops.dense_pe(gauss, 5, 7), ops.dense_pe(gauss, 5, 7, dtype=BF16),
            ops.resize_bilinear(src, (20, 13)), ops.resize_bilinear(src, (5, 4), dtype=BF16)]


@case
def mask_decoder_tail(dev):
    """mask_dot, mask_dot_multi, uncertainty_mlp"""
    B, gh, gw, C = 2, 3, 5, 32
    up, hyper = _n(dev, "tail/up", (B * gh * gw * 16, C)), _n(dev, "tail/hyper", (B, 3, C))
    ws = [_n(dev, f"tail/u{i}", s, 0.2, BF16) for i, s in enumerate([(64, 256), (64,), (16, 64), (16,), (1, 16), (1,)])]
    return [ops.mask_dot(up, hyper[:, 0].contiguous(), B, gh, gw), ops.mask_dot(up.to(BF16), hyper[:, 1].contiguous().to(BF16), B, gh, gw),
            ops.mask_dot_multi(up, hyper, B, gh, gw), ops.mask_dot_multi(up.to(BF16), hyper.to(BF16), B, gh, gw),
            ops.uncertainty_mlp(_n(dev, "tail/emb", (3, 5, 256)), *ws)]


@case
def prompt_kernels(dev):
    """prompt_embed (every label) and mask_downscale (C = 64, mid = 16, a 3 x 5 grid)"""
    nf, C, mid = 32, 64, 16
    coords = torch.from_numpy(synth.synth_uniform("dense_bits/prompt/coords", (6, 2), 0.0, 1024.0)).to(dev)
    sizes = (4 * (mid // 4), mid // 4, mid // 4, mid // 4, mid * mid, mid, mid, mid, C * mid, C)
    ws = [_n(dev, f"prompt/w{i}", (n,), 0.3) for i, n in enumerate(sizes)]
    return [ops.prompt_embed(coords, _i(dev, [-1, 0, 1, 2, 3, 1]), _n(dev, "prompt/gauss", (2, nf)), _n(dev, "prompt/table", (5, 2 * nf)),
                             (1024, 768)),
            ops.mask_downscale(_n(dev, "prompt/mask", (2, 12, 20), 5.0), ws)]


@case
def rope_kernels(dev):
    """rope_table, rope_kv (bf16 and fp16, with caches and a table) and rope_kv_split"""
    T, H, D, Tmax, pos0 = 5, 2, 16, 16, 4
    tab = ops.rope_table(Tmax, D, 10000.0, dev)
    out = list(tab)
    for dt in (BF16, F16):
        qkv = _n(dev, "rope/qkv", (T, 3 * H * D), 1.0, dt)
        kc, vc = torch.zeros(Tmax, H, D, dtype=dt, device=dev), torch.zeros(Tmax, H, D, dtype=dt, device=dev)
        out += [ops.rope_kv(qkv, H, D, pos0, 10000.0, kc, vc, table=tab), kc, vc]
    out.append(ops.rope_kv(_n(dev, "rope/qkv", (T, 3 * H * D), 1.0, BF16), H, D, pos0, 10000.0))
    qs = ops.split_rows(_n(dev, "rope/qkv32", (T, 3 * H * D)))
    caches = tuple(torch.zeros(Tmax, H, D, dtype=BF16, device=dev) for _ in range(4))
    out += [ops.rope_kv_split(qs, H, D, pos0, caches, tab), *caches]
    return out


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def _qkv(dev, tag, B, H, Sq, Sk, D, dtype, Bk=None):
    """q, k, v as [B,H,S,D] views of [B,S,H,D] rows (SAM's layout)"""
    return tuple(_n(dev, f"{tag}/{n}", (b, s, H, D), 1.0, dtype).permute(0, 2, 1, 3)
                 for n, b, s in (("q", B, Sq), ("k", Bk or B, Sk), ("v", Bk or B, Sk)))


def _tabs(dev, tag, side, D, std=0.2):
    return _n(dev, tag + "/th", (2 * side - 1, D), std, BF16), _n(dev, tag + "/tw", (2 * side - 1, D), std, BF16)


@case
def attention_plain(dev):
    """bf16 and fp16, causal with q_pos0, K/V of one batch shared by four query batches"""
    out = []
    for dt in (BF16, F16):
        q, k, v = _qkv(dev, "attn/a", 2, 4, 70, 70, 64, dt)
        out.append(ops.attention(q, k, v, 0.125, prescale_q=dt == F16))
        q, k, v = _qkv(dev, "attn/b", 2, 4, 100, 333, 128, dt)
        out.append(ops.attention(q, k, v, 128 ** -0.5, causal=True, q_pos0=233))
        q, k, v = _qkv(dev, "attn/c", 4, 4, 33, 150, 80, dt, Bk=1)
        out.append(ops.attention(q, k, v, 0.1))
    return out


@case
def attention_windows_relpos(dev):
    """14 x 14 windows, head dim 80: rel= from the dot kernel (bf16), rel_tab= (bf16 and fp16), q_lo= at both levels (fp16)"""
    side, B, H, D = 14, 3, 4, 80
    th, tw = _tabs(dev, "win", side, D)
    q, k, v = _qkv(dev, "win", B, H, side * side, side * side, D, BF16)
    rel = ops.relpos_bias(q, th, tw, side, side)
    out = [*rel, ops.attention(q, k, v, D ** -0.5, rel=rel), ops.attention(q, k, v, D ** -0.5, rel_tab=(ops.relpos_table64(th, tw), side))]
    cat = ops.bf16_to_f16(ops.relpos_tables_cat(th, tw))
    q32 = _n(dev, "win/q32", (B, side * side, H, D)).permute(0, 2, 1, 3)
    qh = q32.to(F16)
    ql = (q32 - qh.float()).to(F16)
    k16, v16 = k.to(F16), v.to(F16)
    out.append(ops.attention(qh, k16, v16, D ** -0.5, rel_tab=(cat, side)))
    out += [ops.attention(qh, k16, v16, D ** -0.5, rel_tab=(cat, side), q_lo=ql, q_lo_level=level) for level in (1, 2)]
    return out


@case
def attention_split_forms(dev):
    """every operand as hi + lo bf16 planes: causal with q_pos0, rel= from relpos_bias_split, rel_tab="""
    def planes(t):  # fp32 [B,S,H,D] -> (hi, lo) [B,H,S,D] views of one [B,S,2,H,D] buffer (the GEMM's split output)
        hi = t.to(BF16)
        buf = torch.stack([hi, (t - hi.float()).to(BF16)], 2).contiguous()
        return buf[:, :, 0].permute(0, 2, 1, 3), buf[:, :, 1].permute(0, 2, 1, 3)

    B, H, D = 2, 4, 128
    (qh, ql), (kh, kl), (vh, vl) = (planes(_n(dev, f"split/{n}", (B, s, H, D))) for n, s in (("q", 70), ("k", 70), ("v", 70)))
    out = [ops.attention_split(qh, ql, kh, kl, vh, vl, D ** -0.5, causal=True)]
    side, B, H, D = 14, 2, 4, 80
    S = side * side
    th, tw = _tabs(dev, "split", side, D, 0.5)
    (qh, ql), (kh, kl), (vh, vl) = (planes(_n(dev, f"split/w{n}", (B, S, H, D))) for n in "qkv")
    rel = ops.relpos_bias_split(qh, ql, th, tw, side, side)
    out += [*rel, ops.attention_split(qh, ql, kh, kl, vh, vl, D ** -0.5, rel=rel),
            ops.attention_split(qh, ql, kh, kl, vh, vl, D ** -0.5, rel_tab=(ops.relpos_table64(th, tw), side))]
    return out


@case
def attention_f32_widths(dev):
    out = []
    for D, Sk in ((16, 65), (128, 65)):
        q, k, v = _qkv(dev, f"f32/{D}", 4, 2, 5, Sk, D, F32, Bk=2)
        out.append(ops.attention_f32(q, k, v, D ** -0.5))
    return out


@case
def relpos_bias_grid(dev):
    """the 64 x 64 grid: the GEMM formulation with its gather (bf16 cat table), and fp16 q with and without a lo plane"""
    side, B, H, D = 64, 1, 2, 80
    th, tw = _tabs(dev, "grid", side, D)
    q32 = _n(dev, "grid/q", (B, side * side, H, D)).permute(0, 2, 1, 3)
    cat = ops.relpos_tables_cat(th, tw)
    cat16 = ops.bf16_to_f16(cat)
    qh = q32.to(F16)
    ql = (q32 - qh.float()).to(F16)
    return [*ops.relpos_bias(q32.to(BF16), th, tw, side, side, cat=cat), *ops.relpos_bias(qh, th, tw, side, side, cat=cat16),
            *ops.relpos_bias(qh, th, tw, side, side, cat=cat16, q_lo=ql)]


# ---- decode attention ------------------------------------------------------------------------------------------------------------------
DH, DD, TMAX = 3, 128, 1024


def _cache(dev, dt, lo=False, B=None):
    """k, v (and their lo planes) [Tmax, H, D], or B copies as slabs"""
    k32, v32 = _n(dev, "dec/k", (TMAX, DH, DD)), _n(dev, "dec/v", (TMAX, DH, DD))
    planes = [k32.to(dt), v32.to(dt)]
    if lo:
        planes += [(k32 - planes[0].float()).to(dt), (v32 - planes[1].float()).to(dt)]
    return [torch.stack([t] * B).contiguous() for t in planes] if B else planes


@case
def decode_attn_one_sequence(dev):
    """bf16 qkv, fp32 qkv on a bf16 cache, an fp16 cache, lo= planes, scratch=; each with a host and a device position"""
    tab = ops.rope_table(TMAX, DD, 10000.0, dev)
    q32 = _n(dev, "dec/q", (1, 3 * DH * DD))
    scratch = ops.decode_attn_scratch(DH, DD, dev)
    out = []
    forms = ((q32.to(BF16), BF16, False, None), (q32, BF16, False, None), (q32, F16, False, None), (q32, BF16, True, None),
             (q32, BF16, False, scratch), (q32, F16, False, scratch))
    for q, dt, lo, scr in forms:
        for pos in (385, _i(dev, [800])):
            c = _cache(dev, dt, lo)
            o = ops.llama_decode_attn(q, c[0], c[1], DH, DD, pos, 10000.0, DD ** -0.5, table=tab, lo=tuple(c[2:]) if lo else None,
                                      scratch=scr)
            p = 385 if isinstance(pos, int) else 800
            out += [o] + [t[p] for t in c]
    out.append(ops.llama_decode_attn(q32, *_cache(dev, BF16), DH, DD, 17, 10000.0, DD ** -0.5))  # no table: the kernel's own cos / sin
    return out


@case
def decode_attn_batch_forms(dev):
    """bf16 / fp32 qkv on bf16 slabs, fp16 slabs, lo= planes; one sequence at Tmax (a zero row)"""
    tab = ops.rope_table(TMAX, DD, 10000.0, dev)
    q32 = _n(dev, "decb/q", (3, 3 * DH * DD))
    pos = [383, 800, TMAX]
    out = []
    for q, dt, lo in ((q32.to(BF16), BF16, False), (q32, BF16, False), (q32, F16, False), (q32, BF16, True)):
        c = _cache(dev, dt, lo, B=3)
        o = ops.llama_decode_attn_batch(q, c[0], c[1], DH, DD, _i(dev, pos), 10000.0, DD ** -0.5, table=tab,
                                        lo=tuple(c[2:]) if lo else None)
        out += [o] + [t[b, pos[b]] for t in c for b in range(2)]
    return out


@case
def decode_attn_batch_prefix_forms(dev):
    tab = ops.rope_table(TMAX, DD, 10000.0, dev)
    q32 = _n(dev, "decp/q", (5, 3 * DH * DD))
    pos = [64, 70, 385, 800, TMAX]
    out = []
    for dt in (BF16, F16):
        kc, vc = _cache(dev, dt, B=5)
        o = ops.llama_decode_attn_batch_prefix(q32, kc, vc, DH, DD, _i(dev, pos), _i(dev, [64]), 10000.0, DD ** -0.5, table=tab,
                                               host_check=(pos, 64))
        out += [o] + [t[b, pos[b]] for t in (kc, vc) for b in range(4)]
    return out


@case
def verify_attn_and_accept(dev):
    tab = ops.rope_table(TMAX, DD, 10000.0, dev)
    qkv = _n(dev, "ver/q", (5, 3 * DH * DD))
    out = []
    for dt in (BF16, F16):
        kc, vc = _cache(dev, dt)
        out += [ops.llama_verify_attn(qkv, kc, vc, DH, DD, _i(dev, [260]), 10000.0, DD ** -0.5, table=tab), kc[260: 265], vc[260: 265]]
    n_acc, tok, pos = _i(dev, [-7]), _i(dev, [-7]), _i(dev, [41])
    ops.spec_accept(_i(dev, [4, 5, 6, 9, 2, 3]), _i(dev, [1, 4, 5, 8, 9, 2]), _i(dev, [5]), n_acc, tok, pos)
    return out + [n_acc, tok, pos]
