"""SAM ViT image encoder, prompt encoder (text, point, box and mask prompts) and two-way mask decoder on the HIP kernels.

Host-side orchestration only (buffers, views, launch order); every FLOP runs in libivlm_hip.so.
Mirrors model/segment_anything/modeling/{image_encoder,prompt_encoder,mask_decoder,transformer,sam}.py of the
reference.  Activations are kept channels-last ([tokens, C]) end to end: LayerNorm2d becomes a row LayerNorm,
the 1x1 / 3x3 / transposed convolutions become GEMMs, and the decoder consumes the encoder output without the
NCHW<->NHWC permutes the reference performs (transformer.py:82-84, mask_decoder.py:141).
"""
from __future__ import annotations

import collections
import functools
import math

import torch

from . import graphs, ops
from .weights import SAM_PREFIX, SamEncCfg

BF16 = torch.bfloat16
F32 = torch.float32


def _dev(t, device):
    return t.to(device=device, dtype=BF16).contiguous()


class _Lin:
    def __init__(self, w, prefix, device, bias=True):
        self.w = _dev(w[prefix + ".weight"].reshape(w[prefix + ".weight"].shape[0], -1), device)
        self.b = _dev(w[prefix + ".bias"], device) if bias and (prefix + ".bias") in w else None

    def __call__(self, x, act="none", residual=None, res_mod=0, out=None, out_f32=False, out_rows=None, a_rows=None,
                 a_split=False, out_split=False):
        return ops.linear(x, self.w, self.b, act=act, residual=residual, res_mod=res_mod, out=out, out_f32=out_f32,
                          out_rows=out_rows, a_rows=a_rows, a_split=a_split, out_split=out_split)


class _LinF32(_Lin):
    """nn.Linear on fp32 activations through the bf16 matrix cores: the input arrives as [hi | lo] bf16 rows
    (ops.split_rows / the split outputs of add_rows) and meets [W | W] (K' = 2K); bias, activation and an fp32 residual in the
    epilogue, fp32 out.  Used where the FLOPs are negligible and the precision is not (the SAM mask decoder)."""

    def __init__(self, w, prefix, device, bias=True):
        super().__init__(w, prefix, device, bias)
        self.w = torch.cat([self.w, self.w], 1).contiguous()

    def __call__(self, x_split, act="none", residual=None):
        return ops.linear(x_split, self.w, self.b, act=act, residual=residual, out_f32=True)


class _LN:
    def __init__(self, w, prefix, device, eps):
        self.w, self.b, self.eps = _dev(w[prefix + ".weight"], device), _dev(w[prefix + ".bias"], device), eps

    def __call__(self, x, gelu=False, out_f32=False, out=None, out_rows=None, fp8_scale=None, out_split=False, out_f16=False):
        return ops.layernorm(x, self.w, self.b, self.eps, gelu=gelu, out_f32=out_f32, out=out, out_rows=out_rows,
                             fp8_scale=fp8_scale, out_split=out_split, out_f16=out_f16)


# ================================================================================================
# image encoder
# ================================================================================================
_F16, _F16_SPLIT = dict(out_f16=True), dict(out_f16=True, out_split=True)
_SPLIT, _SPLIT_A, _SPLIT_AO = dict(out_split=True), dict(a_split=True), dict(a_split=True, out_split=True)

# The MFMA operands of an encoder block per precision mode (SamImageEncoder.precision): the flags of norm1's output, of the q|k|v
# GEMM ("f16q": of its q part), the attention kind, the flags of the proj GEMM, of norm2's output and of the two MLP GEMMs, and
# whether the neck takes [hi | lo] operands.  A GEMM on fp16 operands reads the fp16 copy of its weight (_Block.weight).
_Mode = collections.namedtuple("_Mode", "n1 qkv attn proj n2 lin1 lin2 split_neck")
_MODES = {"default": _Mode({}, {}, "bf16", {}, {}, {}, {}, False),
          "f16": _Mode(_F16, _F16, "f16", {}, _F16, _F16, {}, True),
          "f16q": _Mode(_F16_SPLIT, dict(_F16_SPLIT, a_split=True), "f16q", {}, _F16, _F16, {}, True),
          "parity-fast": _Mode(_SPLIT, _SPLIT_AO, "split", _SPLIT_A, _F16, _F16, {}, True),
          "parity": _Mode(_SPLIT, _SPLIT_AO, "split", _SPLIT_A, _SPLIT, _SPLIT_AO, _SPLIT_A, True)}


class _Block(dict):
    """One encoder block's tensors.  The derived ones are built on first access, i.e. only in a mode that reads them: ``rel_cat``
    ([rel_pos_h ; rel_pos_w], ops.relpos_tables_cat), the fp16 copies ``rel_cat_h``, ``qkv_b_h`` and ``<gemm>_h`` (ops.f16_weight:
    a bf16 weight inside the fp16 normal range converts exactly, one outside it raises), and the rows that fill the padded window
    positions of the split and exact-q q|k|v buffers (``qkv_b_split``, ``q_b_split_h``, ``kv_b_h``)."""

    def __missing__(self, k):
        if k == "rel_cat":
            t = ops.relpos_tables_cat(self["rel_h"], self["rel_w"])
        elif k in ("rel_cat_h", "qkv_b_h"):
            t = ops.bf16_to_f16(self["rel_cat"] if k == "rel_cat_h" else self["qkv"].b)
        elif k in ("qkv_h", "proj_h", "lin1_h", "lin2_h"):
            t = ops.f16_weight(self[k[:-2]].w, k[:-2])
        elif k == "qkv_b_split":
            t = torch.cat([self["qkv"].b, torch.zeros_like(self["qkv"].b)]).contiguous()
        elif k in ("q_b_split_h", "kv_b_h"):
            b = self["qkv_b_h"]
            D = b.numel() // 3
            t = torch.cat([b[:D], torch.zeros_like(b[:D])]).contiguous() if k == "q_b_split_h" else b[D:].contiguous()
        else:
            raise KeyError(k)
        self[k] = t
        return t

    def weight(self, n, a):
        """GEMM n's weight for the A operand a: its fp16 copy for fp16 operands (ops.linear takes both in one type)"""
        return self[n + "_h"] if a.dtype == torch.float16 else self[n].w


class SamImageEncoder:
    """ImageEncoderViT.forward (image_encoder.py:110-125): [V,3,S,S] bf16 -> [V, g*g, 256] bf16 (channels last)."""

    def __init__(self, w, cfg: SamEncCfg, device, prefix=SAM_PREFIX + ".image_encoder"):
        self.cfg, self.device = cfg, device
        self._graphs = graphs.Cache()
        p = prefix
        D = cfg.embed_dim
        self.patch = _Lin(w, p + ".patch_embed.proj", device)
        self.pos_embed = _dev(w[p + ".pos_embed"].reshape(-1, D), device)
        self.blocks = []
        for i in range(cfg.depth):
            bp = f"{p}.blocks.{i}"
            self.blocks.append(_Block(
                glob=i in cfg.global_attn_indexes,
                norm1=_LN(w, bp + ".norm1", device, 1e-6), norm2=_LN(w, bp + ".norm2", device, 1e-6),
                qkv=_Lin(w, bp + ".attn.qkv", device), proj=_Lin(w, bp + ".attn.proj", device),
                rel_h=_dev(w[bp + ".attn.rel_pos_h"], device), rel_w=_dev(w[bp + ".attn.rel_pos_w"], device),
                lin1=_Lin(w, bp + ".mlp.lin1", device), lin2=_Lin(w, bp + ".mlp.lin2", device)))
        self.neck0 = _Lin(w, p + ".neck.0", device, bias=False)
        self.neck1 = _LN(w, p + ".neck.1", device, 1e-6)
        # conv3x3 weight [O, I, ky, kx] -> GEMM weight [O, (ky, kx, I)] matching im2col3x3_nhwc
        w2 = w[p + ".neck.2.weight"]
        self.neck2_w = _dev(w2.permute(0, 2, 3, 1).reshape(w2.shape[0], -1), device)
        self.neck3 = _LN(w, p + ".neck.3", device, 1e-6)
        self._maps = {}
        self._xw = {}  # per (attention kind, view count): the window-ordered q|k|v buffers of the windowed blocks

    def _window_maps(self, V):
        """Row maps of window_partition / window_unpartition (image_encoder.py:263-318) incl. zero padding."""
        if V not in self._maps:
            g, ws = self.cfg.grid, self.cfg.window
            nw = (g + ws - 1) // ws
            gp = nw * ws
            v = torch.arange(V).view(V, 1, 1, 1, 1)
            wy = torch.arange(nw).view(1, nw, 1, 1, 1)
            wx = torch.arange(nw).view(1, 1, nw, 1, 1)
            iy = torch.arange(ws).view(1, 1, 1, ws, 1)
            ix = torch.arange(ws).view(1, 1, 1, 1, ws)
            y, x = wy * ws + iy, wx * ws + ix
            src = (v * g + y) * g + x
            part = torch.where((y < g) & (x < g), src, torch.full_like(src, -1)).reshape(-1)
            yy = torch.arange(g).view(1, g, 1)
            xx = torch.arange(g).view(1, 1, g)
            vv = torch.arange(V).view(V, 1, 1)
            unpart = (((vv * nw + yy // ws) * nw + xx // ws) * ws + yy % ws) * ws + xx % ws
            pad = (part < 0).nonzero().flatten()  # window positions that overhang the grid (zero tokens)
            self._maps[V] = (part.to(torch.int32).to(self.device), unpart.reshape(-1).to(torch.int32).to(self.device),
                             nw, gp, pad.to(torch.int32).to(self.device))
        return self._maps[V]

    def _qkv_buffers(self, kind, V, nwin, device):
        """The q|k|v output of the windowed blocks in window order, one set shared by all of them: [rows, 3D] bf16 / fp16,
        [q hi | q lo] and [k | v] fp16 ("f16q"), [rows, 6D] bf16 = [hi | lo] ("split")."""
        if (kind, V) not in self._xw:
            rows, D = nwin * self.cfg.window ** 2, self.cfg.embed_dim
            shapes = {"bf16": [(3, BF16)], "f16": [(3, torch.float16)], "f16q": [(2, torch.float16)] * 2, "split": [(6, BF16)]}[kind]
            self._xw[(kind, V)] = [torch.empty(rows, n * D, dtype=dt, device=device) for n, dt in shapes]
        return self._xw[(kind, V)]

    # ---- fp8 (OCP e4m3) operands for the four big GEMMs of every block (BASELINE.json configs[4]; opt-in, on top of "default") ----
    # Per-tensor scales: the weights are quantised once (amax / 448); the activation scales (norm1 / attention / norm2 / GELU
    # outputs of every block) are calibrated on one bf16 pass over sample images and then FIXED (values beyond them saturate).
    # The quantisation is fused into the producers: the LayerNorms and the mlp1 GEMM's GELU epilogue write e4m3 directly; only
    # the attention output (bf16 kernel) takes one conversion pass.  Patch embedding, attention and neck stay bf16; the residual
    # stream stays fp32.
    fp8 = False
    _calibrating = False

    def enable_fp8(self, calib_images):
        """calib_images [V,3,S,S]: one bf16 pass records the activation ranges, then the fp8 path is switched on."""
        dev = self.device
        for blk in self.blocks:
            for n in ("qkv", "proj", "lin1", "lin2"):
                q, sc = ops.quantize_fp8(blk[n].w)
                blk[n + "_q"], blk[n + "_s"] = q, sc
            blk["amax"] = {k: torch.zeros(1, dtype=F32, device=dev) for k in ("n1", "att", "n2", "h")}
        self._calibrating = True
        try:
            self._forward(calib_images.to(dev))
        finally:
            self._calibrating = False
        for blk in self.blocks:
            blk["s"] = {k: (v / 448.0).clamp_(min=1e-12) for k, v in blk["amax"].items()}
        self.fp8 = True
        self._graphs.clear()

    # The encoder is ~320 launches (ViT-H, 4 views).  Issued one by one they cost the host ~22 ms - during which the language
    # path, launched after it by the same thread, has not even started (measured: the first 21.9 ms of evaluate() had an idle
    # main stream).  Replayed as ONE HIP graph per input shape the host is free after ~20 us.  Same kernels, same order.
    use_graph = graphs.ON

    def __call__(self, images):
        if not graphs.enabled(self.use_graph, images):
            return self._forward(images)
        key = (tuple(images.shape), self.fp8, self.precision, self.q_lo_level)
        return self._graphs.run(key, self._forward, [images], BF16)

    # ---- precision modes (_MODES; model.InteractVLMForCausalLM.set_precision maps the model's modes onto them) -------------------
    # "default": bf16 MFMA operands.
    # "parity" (fp32-activation arithmetic on the bf16 matrix cores): every activation that "default" rounds to a bf16 MFMA operand
    #   (normed rows, q / k / v, softmax weights, attention output, MLP hidden) is carried as hi + lo bf16 halves (x = hi + lo to
    #   2^-17): the four GEMMs of a block take [hi | lo] rows against the plain weight (each W tile used twice: 2 x the MFMA work),
    #   the attention runs three MFMAs per fragment, rel-pos terms / q scaling / softmax stay fp32.  The bf16 weights are exact in
    #   every mode.  Measured on the headline configuration (ViT-H depth 32, 7B): "default" max |dp| 5.8e-3 against the fp32
    #   oracle, this mode < 1e-3 (bench.py).
    # "parity-fast": "parity" with the MLP's two GEMMs on IEEE fp16 operands - norm2 and the GELU epilogue write halves (11
    #   significant bits: an eighth of the bf16 rounding error, ONE MFMA pass), the bf16 weights convert to fp16 exactly; measured
    #   4.6e-4 end to end at depth 32 against 4.0e-4 with the "parity" encoder, 12 ms less per 4 views
    #   (tools/experiments/diag_precision_modes.py).
    # "f16": EVERY MFMA operand of a block as IEEE fp16 in one pass (norm1 output, q | k | v, softmax weights, attention output,
    #   rel-pos table, norm2 output, GELU hidden) - the bf16 path's launches and FLOPs at an eighth of its operand rounding; the neck
    #   (0.1 % of the FLOPs) takes hi + lo operands.
    # "f16q": "f16" with the "exact q" path: norm1 writes [hi | lo] IEEE halves, q = W_q . (hi + lo) leaves its own GEMM as hi + lo
    #   halves (k | v: a single-pass GEMM on the hi half), the attention takes q = hi + lo in the rel-pos table product (q_lo_level
    #   2: in Q.K^T too, with the softmax weights split for P.V).  q's rounding is the one SAM's decomposed rel-pos terms amplify
    #   (tools/emulate_f16_sites.py: 57 % of the fp16 mode's error variance comes through q), this path removes it for +1/3 of the
    #   q|k|v GEMM's MFMA work.
    precision = "default"
    q_lo_level = 1

    def _attention(self, blk, xn, side, nwin, win=None, fp8=False):
        """Attention.forward (image_encoder.py:235-260) on rows laid out [nwin, side*side, D] -> the attention output [nwin*S, D]
        ([nwin*S, 2D] = [hi | lo] rows for the "split" kind).  win = (unpart, pad, _qkv_buffers): xn is in IMAGE order and the
        block is windowed - the q|k|v GEMM runs on the real rows only and scatters them to their window positions (window_partition
        folded into its epilogue); the rows of the padded window positions, whose input is zero, are the bias: filled, not computed
        (16 % of the rows at 64x64 / 14)."""
        c = self.cfg
        D = c.embed_dim
        H, hd = c.num_heads, D // c.num_heads
        S = side * side
        m = _MODES[self.precision]
        b = blk["qkv"].b
        if fp8:
            gemms = [(functools.partial(ops.linear_fp8, xn, blk["qkv_q"], blk["s"]["n1"], blk["qkv_s"], b), b)]
        elif m.attn == "f16q":  # [q hi | q lo] from the [hi | lo] rows, [k | v] from a single-pass GEMM on the hi half
            w = blk["qkv_h"]
            gemms = [(functools.partial(ops.linear, xn, w[:D], b[:D], **m.qkv), blk["q_b_split_h"]),
                     (functools.partial(ops.linear, xn[:, :D], w[D:], b[D:], out_f16=True), blk["kv_b_h"])]
        else:
            fill = blk["qkv_b_h"] if m.attn == "f16" else (blk["qkv_b_split"] if m.attn == "split" else b)
            gemms = [(functools.partial(ops.linear, xn, blk.weight("qkv", xn), b, **m.qkv), fill)]
        if win is None:
            outs = [gemm() for gemm, _ in gemms]
        else:
            unpart, pad, outs = win
            for (gemm, _), o in zip(gemms, outs):
                gemm(out=o, out_rows=unpart)
            for (_, fill), o in zip(gemms, outs):
                ops.fill_rows(o, pad, fill)
        if m.attn == "split":
            # the fp32 rel-pos terms as arrays: the whole-window split kernel has no LDS left for the table product, and arrays
            # measured faster than the generic split kernel in table mode
            q6 = outs[0].view(nwin, S, 2, 3, H, hd)
            (q, k, v), (q_lo, k_lo, v_lo) = ([q6[:, :, j, i].permute(0, 2, 1, 3) for i in range(3)] for j in range(2))
            rel = ops.relpos_bias_split(q, q_lo, blk["rel_h"], blk["rel_w"], side, side)
            return ops.attention_split(q, q_lo, k, k_lo, v, v_lo, hd ** -0.5, rel=rel)
        if m.attn == "f16q":
            q4, kv4 = (t.view(nwin, S, 2, H, hd) for t in outs)
            q, q_lo, k, v = (t.permute(0, 2, 1, 3) for t in (q4[:, :, 0], q4[:, :, 1], kv4[:, :, 0], kv4[:, :, 1]))
            lv = self.q_lo_level
        else:
            qkv5 = outs[0].view(nwin, S, 3, H, hd)
            q, k, v = (qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
            q_lo, lv = None, 1
        tab = blk["rel_cat_h"] if q.dtype == torch.float16 else blk["rel_cat"]
        # table mode: the attention kernel computes the decomposed rel-pos terms itself (one small MFMA product per query tile
        # against the [rel_pos_h ; rel_pos_w] table) - no relpos pass, no [B*H, S, 2 side] fp32 arrays.  Windows and the 64 x 64
        # grid at head dim 80; level 2 of the exact q path has no table mode on the grid.
        if hd == 80 and (2 * side <= 32 or (side == 64 and lv < 2)):
            o = ops.attention(q, k, v, hd ** -0.5, rel_tab=(tab, side), q_lo=q_lo, q_lo_level=lv)
        else:
            rel = ops.relpos_bias(q, blk["rel_h"], blk["rel_w"], side, side, cat=tab, q_lo=q_lo)
            o = ops.attention(q, k, v, hd ** -0.5, rel=rel, q_lo=q_lo if lv == 2 else None, q_lo_level=lv)
        return o.permute(0, 2, 1, 3).reshape(nwin * S, H * hd)

    def _block(self, blk, x, V, nwin, win, fp8=False):
        """Block.forward (image_encoder.py:177-193) on the fp32 residual stream x [V*g*g, D].  A windowed block runs both attention
        GEMMs on the g*g real rows of every view only: window_partition is folded into the q|k|v GEMM's scatter epilogue (_attention)
        and window_unpartition + shortcut into the proj GEMM's gather prologue, in place (its A rows are gathered from their window
        positions; the rows of the padded window grid are never computed)."""
        c = self.cfg
        glob = blk["glob"]
        side, nw_, win = (c.grid, V, None) if glob else (c.window, nwin, win)
        a_rows = None if glob else win[0]
        if fp8:  # e4m3 operands for qkv / proj / mlp1 / mlp2 (same dataflow as the bf16 block)
            sc = blk["s"]
            a = self._attention(blk, blk["norm1"](x, fp8_scale=sc["n1"]), side, nw_, win, fp8=True)
            aq = ops.gather_rows(a, out_kind="fp8", scale=sc["att"])
            x = ops.linear_fp8(aq, blk["proj_q"], sc["att"], blk["proj_s"], blk["proj"].b, residual=x, out=x, a_rows=a_rows)
            hq = blk["norm2"](x, fp8_scale=sc["n2"])
            h8 = ops.linear_fp8(hq, blk["lin1_q"], sc["n2"], blk["lin1_s"], blk["lin1"].b, act="gelu", out_kind="fp8",
                                scale_out=sc["h"])
            return ops.linear_fp8(h8, blk["lin2_q"], sc["h"], blk["lin2_s"], blk["lin2"].b, residual=x, out=x)
        m = _MODES[self.precision]
        cal = blk.get("amax") if self._calibrating and self.precision == "default" else None  # (enable_fp8)
        xn = blk["norm1"](x, **m.n1)
        if cal:
            ops.amax(xn, cal["n1"])
        a = self._attention(blk, xn, side, nw_, win)
        if cal:
            ops.amax(a, cal["att"])
        x = ops.linear(a, blk.weight("proj", a), blk["proj"].b, residual=x, out_f32=True, out=None if glob else x, a_rows=a_rows,
                       **m.proj)
        xn2 = blk["norm2"](x, **m.n2)
        h = ops.linear(xn2, blk.weight("lin1", xn2), blk["lin1"].b, act="gelu", **m.lin1)
        if cal:
            ops.amax(xn2, cal["n2"])
            ops.amax(h, cal["h"])
        return ops.linear(h, blk.weight("lin2", h), blk["lin2"].b, residual=x, out_f32=True, **m.lin2)

    def _forward(self, images):
        """The residual stream x is fp32 (GEMM residual epilogues write it, the LayerNorms read it); the MFMA operands are those
        of the precision mode, or e4m3 (fp8, on top of "default")."""
        c = self.cfg
        V = images.shape[0]
        g = c.grid
        m = _MODES[self.precision]
        cols = ops.im2col_nchw(images.to(BF16).contiguous(), c.patch, c.patch)  # (bf16 pixels x bf16 weights: exact products)
        x = self.patch(cols, residual=self.pos_embed, res_mod=g * g, out_f32=True)  # + pos_embed broadcast over views
        part, unpart, nw, gp, pad = self._window_maps(V)
        nwin = V * nw * nw
        win = (unpart, pad, self._qkv_buffers(m.attn, V, nwin, x.device))
        fp8 = self.fp8 and self.precision == "default"
        for blk in self.blocks:
            x = self._block(blk, x, V, nwin, win, fp8)
        if m.split_neck:
            y = self.neck0(ops.gather_rows(x, out_kind="split"), out_f32=True, a_split=True)
            y = self.neck1(y, out_split=True)  # [V*g*g, 2 * 256]
            y = ops.linear(ops.im2col3x3_nhwc_split(y, V, g, g, c.out_chans), self.neck2_w, out_f32=True, a_split=True)
        else:
            y = self.neck1(self.neck0(ops.gather_rows(x, out_kind="bf16")))
            y = ops.linear(ops.im2col3x3_nhwc(y.view(V, g, g, c.out_chans)), self.neck2_w)
        return self.neck3(y, out_f32=True).view(V, g * g, c.out_chans)  # fp32: the mask decoder keeps fp32 activations


# ================================================================================================
# prompt encoder (text-embedding path) + mask decoder + postprocess
# ================================================================================================
class SamMaskDecoder:
    """PromptEncoder.forward(text_embeds=...) + MaskDecoder.forward(multimask_output=False)
    (prompt_encoder.py:140-186, mask_decoder.py:75-164, transformer.py:62-242).

    Precision: this stage is 15 GFLOP of the image's 27 TFLOP and it writes the mask logits, so it runs with fp32 activations
    end to end: every nn.Linear / transposed conv takes its input as hi + lo bf16 rows against [W | W] (``_LinF32``: an
    fp32-activation GEMM on the bf16 matrix cores, weights exactly the checkpoint's bf16), the attentions run in fp32
    (``ops.attention_f32``), LayerNorms and the hypernetwork product read and write fp32."""

    def __init__(self, w, device, grid=64, prefix=SAM_PREFIX, decoder="mask_decoder"):
        """decoder: the attribute name of the decoder module to load ('-DifDe' checkpoints also carry 'human_mask_decoder' and
        'object_mask_decoder', separately trained copies: InteractVLM.py:114-121); the prompt encoder is shared."""
        self.device, self.grid = device, grid
        self._graphs = graphs.Cache()
        pe, md = prefix + ".prompt_encoder", prefix + "." + decoder
        self.C = C = w[md + ".iou_token.weight"].shape[1]
        f32 = lambda t: t.to(device=device, dtype=BF16).to(F32).contiguous()  # the checkpoint's bf16 values, held as fp32
        self.no_mask = f32(w[pe + ".no_mask_embed.weight"].reshape(1, C))
        gauss = w[pe + ".pe_layer.positional_encoding_gaussian_matrix"].to(device=device, dtype=torch.float32).contiguous()
        self.key_pe = ops.dense_pe(gauss, grid, grid)  # fp32 [g*g, C] constant: computed once, not per call
        self.out_tokens = f32(torch.cat([w[md + ".iou_token.weight"], w[md + ".mask_tokens.weight"]], 0))
        self.n_mask = w[md + ".mask_tokens.weight"].shape[0]
        tp = md + ".transformer"

        def attn(p):
            return dict(q=_LinF32(w, p + ".q_proj", device), k=_LinF32(w, p + ".k_proj", device),
                        v=_LinF32(w, p + ".v_proj", device), o=_LinF32(w, p + ".out_proj", device))

        self.layers = []
        i = 0
        while f"{tp}.layers.{i}.norm1.weight" in w:
            lp = f"{tp}.layers.{i}"
            self.layers.append(dict(
                self_attn=attn(lp + ".self_attn"), t2i=attn(lp + ".cross_attn_token_to_image"),
                i2t=attn(lp + ".cross_attn_image_to_token"),
                norm1=_LN(w, lp + ".norm1", device, 1e-5), norm2=_LN(w, lp + ".norm2", device, 1e-5),
                norm3=_LN(w, lp + ".norm3", device, 1e-5), norm4=_LN(w, lp + ".norm4", device, 1e-5),
                lin1=_LinF32(w, lp + ".mlp.lin1", device), lin2=_LinF32(w, lp + ".mlp.lin2", device)))
            i += 1
        self.final_attn = attn(tp + ".final_attn_token_to_image")
        self.norm_final = _LN(w, tp + ".norm_final_attn", device, 1e-5)
        # ConvTranspose2d(k=2,s=2) as GEMM: weight [ci, co, dy, dx] -> [(dy, dx, co), ci]; bias tiled over (dy,dx)
        w0 = w[md + ".output_upscaling.0.weight"]
        u0 = _dev(w0.permute(2, 3, 1, 0).reshape(-1, w0.shape[0]), device)
        self.up0_w = torch.cat([u0, u0], 1).contiguous()
        self.up0_b = _dev(w[md + ".output_upscaling.0.bias"].repeat(4), device)
        self.up_ln = _LN(w, md + ".output_upscaling.1", device, 1e-6)
        w1 = w[md + ".output_upscaling.3.weight"]
        u1 = _dev(w1.permute(2, 3, 1, 0).reshape(-1, w1.shape[0]), device)
        self.up1_w = torch.cat([u1, u1], 1).contiguous()
        self.up1_b = _dev(w[md + ".output_upscaling.3.bias"].repeat(4), device)
        self.c_mid, self.c_up = w0.shape[1], w1.shape[1]
        self.hyper0 = [_LinF32(w, f"{md}.output_hypernetworks_mlps.0.layers.{j}", device) for j in range(3)]
        self.iou = [_LinF32(w, f"{md}.iou_prediction_head.layers.{j}", device) for j in range(3)]
        # the point / box / mask prompts and the multi-mask output (encode_prompts, predict_masks): all hypernetworks (hyper[0] is
        # hyper0), the Gaussian matrix unrounded, the label table of ops.prompt_embed [negative point ; positive point ; box corner 0 ;
        # box corner 1 ; not-a-point] and the ten tensors of mask_downscaling in the checkpoint's layouts
        self.hyper = [self.hyper0] + [[_LinF32(w, f"{md}.output_hypernetworks_mlps.{m}.layers.{j}", device) for j in range(3)]
                                      for m in range(1, self.n_mask)]
        self.gauss = gauss
        self.point_table = f32(torch.cat([w[f"{pe}.point_embeddings.{i}.weight"].reshape(1, C) for i in range(4)]
                                         + [w[pe + ".not_a_point_embed.weight"].reshape(1, C)], 0))
        self.mask_down = [f32(w[f"{pe}.mask_downscaling.{n}"].reshape(-1)) for n in
                          ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias")]
        self.input_size = (16 * grid, 16 * grid)  # PromptEncoder.input_image_size: 16 input pixels per grid cell (build_sam.py)

    def _attn(self, a, q_split, k_split, v_split, B, Sq, Sk, heads=8, kv_batch=None):
        """Attention.forward (transformer.py:220-242). *_split are [B*S, 2C] hi|lo rows -> fp32 [B*Sq, inner] (before out_proj)."""
        q, k, v = a["q"](q_split), a["k"](k_split), a["v"](v_split)
        inner = q.shape[-1]
        d = inner // heads
        Bk = B if kv_batch is None else kv_batch
        q4 = q.view(B, Sq, heads, d).permute(0, 2, 1, 3)
        k4 = k.view(Bk, Sk, heads, d).permute(0, 2, 1, 3)
        v4 = v.view(Bk, Sk, heads, d).permute(0, 2, 1, 3)
        o = ops.attention_f32(q4, k4, v4, 1.0 / math.sqrt(d))
        return ops.split_rows(o.permute(0, 2, 1, 3).reshape(B * Sq, inner))

    # The decoder chain (prompt tokens -> two-way transformer -> upscaler -> hypernetwork dot -> IoU head) is ~200 launches of
    # 3-30 us kernels with no host decision inside: replayed as ONE HIP graph per (views, tokens) shape (BASELINE.json
    # configs[4]: "fused SAM decoder in one hipGraph").  Same kernels, same order: bit-identical to the eager chain.
    use_graph = graphs.ON

    def __call__(self, image_embeddings, text_embeds):
        if not graphs.enabled(self.use_graph, image_embeddings):
            return self._forward(image_embeddings, text_embeds)
        key = (tuple(image_embeddings.shape), image_embeddings.dtype, tuple(text_embeds.shape), text_embeds.dtype)
        return self._graphs.run(key, self._forward, [image_embeddings, text_embeds])

    def _forward(self, image_embeddings, text_embeds):
        """image_embeddings [V, g*g, C] fp32 or bf16 (channels last); text_embeds [1, T, C] (the views as TOKENS)
        -> low_res_masks f32 [V,1,4g,4g], iou f32 [V,1].

        Batch semantics follow torch broadcasting in the reference exactly: one token set of
        5+T tokens; the first self-attention sees batch 1, every later op batch V.  We carry V identical copies
        from the start (same numbers) so that every kernel sees a fixed batch of V."""
        V, HW, C = image_embeddings.shape
        g = self.grid
        assert text_embeds.shape[0] == 1, "n_seg > 1 with multi-view mis-broadcasts in the reference (SURVEY §7)"
        tokens = torch.cat([self.out_tokens, text_embeds[0].to(F32)], dim=0)  # [Nt, C]
        Nt = tokens.shape[0]
        query_pe = tokens.unsqueeze(0).expand(V, Nt, C).reshape(V * Nt, C).contiguous()
        keys = ops.add_rows(image_embeddings.reshape(V * HW, C).contiguous(), self.no_mask, out_kind="f32")  # src + dense
        hs, keys = self._transformer(query_pe, keys, V, Nt, HW)
        sp = ops.split_rows
        iou_tok = hs[:, 0, :].contiguous()
        mask_tok0 = hs[:, 1, :].contiguous()  # mask token 0: multimask_output=False keeps masks[:, 0:1]
        u = self._upscale(keys)
        h = self.hyper0[2](sp(self.hyper0[1](sp(self.hyper0[0](sp(mask_tok0), act="relu")), act="relu")))  # [V, 32]
        low = ops.mask_dot(u, h, V, g, g)  # f32 [V, 4g, 4g]
        iou = self.iou[2](sp(self.iou[1](sp(self.iou[0](sp(iou_tok), act="relu")), act="relu")))
        return low.unsqueeze(1), iou[:, 0:1]

    def _transformer(self, query_pe, keys, V, Nt, HW):
        """TwoWayTransformer.forward (transformer.py:62-107) + norm_final_attn for V token sets of Nt tokens: query_pe fp32 [V*Nt, C]
        (the tokens: they are their own positional encoding), keys fp32 [V*HW, C] (src + dense) -> (hs fp32 [V, Nt, C], keys)."""
        queries = query_pe
        key_pe = self.key_pe  # [HW, C], broadcast over V by row modulo
        sp = ops.split_rows
        for li, L in enumerate(self.layers):
            if li == 0:  # skip_first_layer_pe: queries = self_attn(q=k=v=queries), no residual
                qs = sp(queries)
                queries = L["self_attn"]["o"](self._attn(L["self_attn"], qs, qs, qs, V, Nt, Nt))
            else:
                q = ops.add_rows(queries, query_pe, out_kind="split")
                sa = self._attn(L["self_attn"], q, q, sp(queries), V, Nt, Nt)
                queries = L["self_attn"]["o"](sa, residual=queries)
            queries = L["norm1"](queries, out_f32=True)
            q = ops.add_rows(queries, query_pe, out_kind="split")
            k = ops.add_rows(keys, key_pe, out_kind="split")
            ca = self._attn(L["t2i"], q, k, sp(keys), V, Nt, HW)
            queries = L["norm2"](L["t2i"]["o"](ca, residual=queries), out_f32=True)
            mlp = L["lin2"](sp(L["lin1"](sp(queries), act="relu")), residual=queries)
            queries = L["norm3"](mlp, out_f32=True)
            q = ops.add_rows(queries, query_pe, out_kind="split")
            ia = self._attn(L["i2t"], k, q, sp(queries), V, HW, Nt)  # image attends to tokens (q=k_img, k=q_tok)
            keys = L["norm4"](L["i2t"]["o"](ia, residual=keys), out_f32=True)
        q = ops.add_rows(queries, query_pe, out_kind="split")
        k = ops.add_rows(keys, key_pe, out_kind="split")
        fa = self._attn(self.final_attn, q, k, sp(keys), V, Nt, HW)
        hs = self.norm_final(self.final_attn["o"](fa, residual=queries), out_f32=True)
        return hs.view(V, Nt, hs.shape[-1]), keys

    def _upscale(self, keys):
        """output_upscaling: ConvT(256->64) -> LayerNorm2d -> GELU -> ConvT(64->32) -> GELU, as GEMMs on pixels: keys fp32 [V*HW, C] ->
        fp32 [V*HW*4, (dy2,dx2,32)], the layout ops.mask_dot reads"""
        sp = ops.split_rows
        u = ops.linear(sp(keys), self.up0_w, self.up0_b, out_f32=True)  # [V*HW, (dy,dx,64)]
        u = self.up_ln(u.view(-1, self.c_mid), gelu=True, out_f32=True)  # per output pixel over 64 channels
        return ops.linear(sp(u), self.up1_w, self.up1_b, act="gelu", out_f32=True)  # [V*HW*4, (dy2,dx2,32)]

    # ---- point / box / mask prompts, multi-mask output (prompt_encoder.py:78-114, 140-186; mask_decoder.py:75-164) --------------------
    def encode_prompts(self, points=None, labels=None, boxes=None, mask_input=None):
        """PromptEncoder.forward(points=(points, labels), boxes=boxes, masks=mask_input): points fp32 [B,N,2] as (x, y) in the padded
        input frame with labels [B,N] (1 positive, 0 negative, -1 not a point), boxes fp32 [B,4] (x0, y0, x1, y1), mask_input fp32
        [B,1,4g,4g] -> (sparse fp32 [B,N',C], dense fp32 [B,g*g,C] or None for no mask).  Token order of the reference: the points,
        then the pad point (label -1) only when there is no box, then the two box corners."""
        B = check_prompts(points, labels, boxes, mask_input, 4 * self.grid)
        dev = self.device
        coords, labs = [], []
        if points is not None:
            coords.append(points.to(dev, F32))
            labs.append(labels.to(dev, torch.int32))
            if boxes is None:
                coords.append(torch.zeros(B, 1, 2, dtype=F32, device=dev))
                labs.append(torch.full((B, 1), -1, dtype=torch.int32, device=dev))
        if boxes is not None:
            coords.append(boxes.to(dev, F32).reshape(B, 2, 2))
            labs.append(torch.tensor([2, 3], dtype=torch.int32, device=dev).expand(B, 2))
        if coords:
            coords, labs = torch.cat(coords, 1).contiguous(), torch.cat(labs, 1).contiguous()
            sparse = ops.prompt_embed(coords, labs, self.gauss, self.point_table, self.input_size).view(B, labs.shape[1], self.C)
        else:
            sparse = torch.empty(B, 0, self.C, dtype=F32, device=dev)
        dense = None
        if mask_input is not None:
            m = mask_input.to(dev, F32).reshape(B, 4 * self.grid, 4 * self.grid).contiguous()
            dense = ops.mask_downscale(m, self.mask_down, eps=1e-6)
        return sparse, dense

    def predict_masks(self, image_embedding, sparse, dense=None, multimask_output=True):
        """MaskDecoder.forward for B prompt sets on ONE image: image_embedding [g*g, C] fp32 or bf16 (channels last), sparse fp32
        [B,N,C], dense fp32 [B,g*g,C] or None (the no-mask embedding) -> (low_res fp32 [B,M,4g,4g], iou fp32 [B,M]): mask tokens 1..3
        with multimask_output, else token 0 (mask_decoder.py:105-111) - slices of one [B,4,...] result, which is replayed as one HIP
        graph per (B, N, dense or not) like the text path (``use_graph``; the same kernels in the same order as the eager chain)."""
        low, iou = self._predict_all(image_embedding, sparse, dense, graph=True)
        return (low[:, 1:], iou[:, 1:]) if multimask_output else (low[:, 0:1], iou[:, 0:1])

    def _predict_all(self, image_embedding, sparse, dense, graph=False):
        """all mask tokens: (low_res fp32 [B,n_mask,4g,4g], iou fp32 [B,n_mask]).  The image embedding and key_pe are repeated over the
        B prompts (mask_decoder.py:137-139) by the row modulo of ops.add_rows; every prompt carries 5 + N tokens.  graph: replay
        where graphs are enabled, else the eager chain."""
        B, N = check_decoder_inputs(self.grid, self.C, self.n_mask, image_embedding, sparse, dense)
        inputs = [image_embedding, sparse] + ([] if dense is None else [dense])
        if graph and graphs.enabled(self.use_graph, *inputs):
            key = ("prompts", B, N, dense is not None, image_embedding.dtype)
            return self._graphs.run(key, self._predict_chain, inputs)
        return self._predict_chain(*inputs)

    def _predict_chain(self, image_embedding, sparse, dense=None):
        g, C = self.grid, self.C
        HW = g * g
        B, N = sparse.shape[0], sparse.shape[1]
        Nt = 1 + self.n_mask + N
        tokens = torch.cat([self.out_tokens.unsqueeze(0).expand(B, -1, -1), sparse], dim=1).reshape(B * Nt, C).contiguous()
        if dense is None:  # no_mask_embed expanded over the grid, as the reference hands it to the decoder
            dense = self.no_mask.expand(B * HW, C)
        keys = ops.add_rows(dense.reshape(B * HW, C).contiguous(), image_embedding.contiguous(), out_kind="f32")  # dense + src[row % HW]
        hs, keys = self._transformer(tokens, keys, B, Nt, HW)
        sp = ops.split_rows
        u = self._upscale(keys)
        hyper = torch.stack([mlp[2](sp(mlp[1](sp(mlp[0](sp(hs[:, 1 + m, :].contiguous()), act="relu")), act="relu")))
                             for m, mlp in enumerate(self.hyper)], dim=1).contiguous()  # [B, n_mask, 32]
        low = ops.mask_dot_multi(u, hyper, B, g, g)  # f32 [B, n_mask, 4g, 4g]
        iou_tok = hs[:, 0, :].contiguous()
        iou = self.iou[2](sp(self.iou[1](sp(self.iou[0](sp(iou_tok), act="relu")), act="relu")))
        return low, iou


def check_decoder_inputs(grid, C, n_mask, image_embedding, sparse, dense):
    """The argument checks of SamMaskDecoder.predict_masks, before the library loads -> (B, N)"""
    HW = grid * grid
    if not isinstance(sparse, torch.Tensor) or sparse.dim() != 3 or sparse.shape[-1] != C or sparse.shape[0] < 1 or sparse.dtype != F32:
        raise ValueError(f"sparse: expected float32 [B,N,{C}], got {_describe(sparse)}")
    B, N = sparse.shape[0], sparse.shape[1]
    if not isinstance(image_embedding, torch.Tensor) or tuple(image_embedding.shape) != (HW, C) or image_embedding.dtype not in (F32, BF16):
        raise ValueError(f"image_embedding: expected ONE image's float32 or bfloat16 [{HW},{C}], got {_describe(image_embedding)}")
    if dense is not None and (not isinstance(dense, torch.Tensor) or tuple(dense.shape) != (B, HW, C) or dense.dtype != F32):
        raise ValueError(f"dense: expected float32 [{B},{HW},{C}] or None, got {_describe(dense)}")
    if n_mask > 4:
        raise ValueError(f"{n_mask} mask tokens: mask_dot_multi takes up to 4")
    return B, N


def _describe(t):
    return f"{t.dtype} {tuple(t.shape)}".replace("torch.", "") if isinstance(t, torch.Tensor) else type(t).__name__


def check_prompts(points, labels, boxes, mask_input, mask_side, batch=True):
    """The argument checks of a prompt set (SamMaskDecoder.encode_prompts, SamPredictor), all before the library loads -> B.
    batch: [B,N,2] / [B,N] / [B,4] / [B,1,S,S]; else one prompt set, [N,2] / [N] / [4] / [1,S,S]."""
    r = 1 if batch else 0
    lead = "[B," if batch else "["
    for t, name in ((points, "point_coords"), (labels, "point_labels"), (boxes, "boxes" if batch else "box"), (mask_input, "mask_input")):
        if t is not None and not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
    if points is None and boxes is None and mask_input is None:
        if labels is not None:
            raise ValueError("point_labels given without point_coords")
        raise ValueError("no prompt: give point_coords with point_labels, a box or a mask_input")
    if (points is None) != (labels is None):
        raise ValueError("point_labels given without point_coords" if points is None else "point_coords given without point_labels")
    sizes = []
    if points is not None:
        if points.dim() != r + 2 or points.shape[-1] != 2 or points.shape[-2] < 1 or not points.is_floating_point():
            raise ValueError(f"point_coords: expected floating-point {lead}N,2] with N >= 1, got {_describe(points)}")
        if tuple(labels.shape) != tuple(points.shape[:-1]) or labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError(f"point_labels: expected integer {lead}N] = {tuple(points.shape[:-1])}, got {_describe(labels)}")
        sizes.append((points.shape[0] if batch else 1, "point_coords"))
    if boxes is not None:
        if boxes.dim() != r + 1 or boxes.shape[-1] != 4 or not boxes.is_floating_point():
            raise ValueError(f"{'boxes' if batch else 'box'}: expected floating-point {lead}4], got {_describe(boxes)}")
        sizes.append((boxes.shape[0] if batch else 1, "boxes"))
    if mask_input is not None:
        if mask_input.dim() != r + 3 or tuple(mask_input.shape[r:]) != (1, mask_side, mask_side) or not mask_input.is_floating_point():
            raise ValueError(f"mask_input: expected floating-point {lead}1,{mask_side},{mask_side}], got {_describe(mask_input)}")
        sizes.append((mask_input.shape[0] if batch else 1, "mask_input"))
    B = sizes[0][0]
    for b, name in sizes:
        if b != B or b < 1:
            raise ValueError(f"{name}: {b} prompt sets, {sizes[0][1]} has {B}")
    return B


def postprocess_masks(low_res, input_size, original_size, img_size=1024, apply_sigmoid=False, sigmoid_gt=None, ignore_label=-1.0):
    """Sam.postprocess_masks (sam.py:137-172) (+ the masked sigmoid of InteractVLM.py:452-456 when sigmoid_gt is given)."""
    return ops.postprocess_masks(low_res.contiguous(), input_size, original_size, img_size, apply_sigmoid, sigmoid_gt, ignore_label)
