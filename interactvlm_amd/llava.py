"""CLIP ViT-L/14 tower + mm_projector + LLaMA decoder (KV-cached) on the HIP kernels.

Mirrors the arithmetic the reference gets from HF ``CLIPVisionModel`` / ``LlamaModel`` through
model/llava/model/{llava_arch.py, language_model/llava_llama.py, multimodal_encoder/clip_encoder.py}.
MI355X-first differences (same numbers, less work):
  * CLIP is encoded ONCE per image; the reference re-encodes it for every generated token
    (InteractVLM.py:128 use_cache=False -> llava_arch.py:98-123 on every step);
  * decode uses a KV cache (the reference re-runs the full prefix each step);
  * q/k/v and gate/up projections are fused GEMMs over concatenated / row-interleaved weights, SwiGLU and
    residual adds live in GEMM epilogues, image features are written straight into the LLM input buffer.
"""
from __future__ import annotations

import collections
import os

import torch

from . import _lib, graphs, ops
from .sam import _LN, _Lin, _dev
from .weights import CLIP_PREFIX, ClipCfg, LlamaCfg

BF16 = torch.bfloat16
F32 = torch.float32

# a captured decode step (Llama._graphs): batched (decode_graph_batch) or not, sequences per step, and what selects its launches;
# verify: a speculative verify pass of this instance's sequence (verify_graph, B = rows per pass); prefix: the batched step whose
# attention reads a shared prompt prefix once for all sequences (decode_graph_batch(prefix=...))
_GraphKey = collections.namedtuple("_GraphKey", "batched B precision packed fp8 fused verify prefix", defaults=(False, False))


class ClipTower:
    """CLIPVisionTower.forward + feature_select('patch', layer -2) (clip_encoder.py:31-60)."""

    def __init__(self, w, cfg: ClipCfg, device, prefix=CLIP_PREFIX):
        self.cfg, self.device = cfg, device
        self._graphs = graphs.Cache()
        self._patch_rows = {}
        e = prefix + ".embeddings"
        K = 3 * cfg.patch * cfg.patch
        self.kpad = ((K + 63) // 64) * 64
        pw = w[e + ".patch_embedding.weight"].reshape(cfg.hidden, K)
        self.patch_w = _dev(torch.nn.functional.pad(pw, (0, self.kpad - K)), device)
        pos = w[e + ".position_embedding.weight"]
        self.pos = _dev(pos, device)
        self.cls_row = (w[e + ".class_embedding"].float() + pos[0].float()).reshape(1, -1).to(device).contiguous()  # fp32
        self.pre_ln = _LN(w, prefix + ".pre_layrnorm", device, cfg.eps)
        n_run = cfg.layers + 1 + cfg.select_layer if cfg.select_layer < 0 else cfg.select_layer
        self.layers = []
        for i in range(n_run):  # hidden_states[-2] is the output of layer L-1: the last layer is never needed
            p = f"{prefix}.encoder.layers.{i}"
            qkv_w = torch.cat([w[f"{p}.self_attn.{n}_proj.weight"] for n in "qkv"], 0)
            qkv_b = torch.cat([w[f"{p}.self_attn.{n}_proj.bias"] for n in "qkv"], 0)
            self.layers.append(dict(
                ln1=_LN(w, p + ".layer_norm1", device, cfg.eps), ln2=_LN(w, p + ".layer_norm2", device, cfg.eps),
                qkv_w=_dev(qkv_w, device), qkv_b=_dev(qkv_b, device), out=_Lin(w, p + ".self_attn.out_proj", device),
                fc1=_Lin(w, p + ".mlp.fc1", device), fc2=_Lin(w, p + ".mlp.fc2", device)))

    use_graph = graphs.ON  # replay the tower as one HIP graph (it is ~250 launches of 5-15 us kernels: launch-bound)

    def __call__(self, images):
        """images [B,3,S,S] bf16 -> patch features [B, T-1, hidden]."""
        if not graphs.enabled(self.use_graph, images):
            return self._forward(images)
        return self._graphs.run((images.shape[0], self.precision, self.fp8), self._forward, [images], BF16)

    # "parity": fp32-activation arithmetic (hi + lo bf16 operands), see SamImageEncoder.precision; "f16": every MFMA operand as
    # IEEE fp16 (one pass, an eighth of the bf16 operand rounding; fp16 copies of the weights made on first use)
    precision = "default"

    def _f16(self, L):
        if "qkv_h" not in L:
            L["qkv_h"] = ops.f16_weight(L["qkv_w"], "clip qkv")
            for n in ("out", "fc1", "fc2"):
                L[n + "_h"] = ops.f16_weight(L[n].w, "clip " + n)
        return L

    # ---- fp8 (OCP e4m3) operands for the four GEMMs of every layer (BASELINE.json configs[4]; opt-in): per-tensor scales, the
    # weights quantised once, the activation ranges calibrated on one bf16 pass over calibration images and then fixed.
    fp8 = False
    _calibrating = False

    def enable_fp8(self, calib_images):
        dev = self.device
        for L in self.layers:
            for n, w_ in (("qkv", L["qkv_w"]), ("out", L["out"].w), ("fc1", L["fc1"].w), ("fc2", L["fc2"].w)):
                L[n + "_q"], L[n + "_s"] = ops.quantize_fp8(w_)
            L["amax"] = {k: torch.zeros(1, dtype=F32, device=dev) for k in ("y1", "a", "y2", "h")}
        self._calibrating = True
        try:
            self._forward(calib_images.to(dev))
        finally:
            self._calibrating = False
        for L in self.layers:
            L["s"] = {k: (v / 448.0).clamp_(min=1e-12) for k, v in L["amax"].items()}
        self.fp8 = True
        self._graphs.clear()

    def _attention(self, qkv, B, split=False):
        """softmax(q k^T * scale) v of B images on their q|k|v rows [B*T, 3*hidden] -> the attention rows [B*T, hidden] in qkv's
        dtype; split: [hi | lo] rows [B*T, 6*hidden] -> [B*T, 2*hidden] (fp32-activation attention, ops.attention_split)"""
        c = self.cfg
        T, H, hd = c.tokens, c.heads, c.hidden // c.heads
        if split:
            q6 = qkv.view(B, T, 2, 3, H, hd)
            (q, k, v), (q_lo, k_lo, v_lo) = ([q6[:, :, j, i].permute(0, 2, 1, 3) for i in range(3)] for j in range(2))
            return ops.attention_split(q, q_lo, k, k_lo, v, v_lo, hd ** -0.5, prescale_q=True)
        q, k, v = (qkv.view(B, T, 3, H, hd)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        return ops.attention(q, k, v, hd ** -0.5, prescale_q=True).permute(0, 2, 1, 3).reshape(B * T, c.hidden)

    def _forward(self, images):
        """-> penultimate-layer patch features, bf16 [B, T-1, hidden] (the mm_projector's MFMA operand; "parity" and "f16"
        precision: [B, T-1, 2*hidden] = [hi | lo] rows).  The residual stream is fp32 between the GEMMs (residual epilogues write
        fp32, the LayerNorms read it)."""
        c = self.cfg
        B = images.shape[0]
        T = c.tokens
        cols = ops.im2col_nchw(images.to(BF16).contiguous(), c.patch, c.patch, self.kpad)  # [B*(T-1), kpad]
        x = torch.empty(B, T, c.hidden, dtype=F32, device=images.device)
        for b in range(B):  # patch GEMM writes rows 1..T-1 and adds their position embeddings in the epilogue
            ops.linear(cols[b * (T - 1): (b + 1) * (T - 1)], self.patch_w, residual=self.pos[1:], out=x[b, 1:])
            ops.gather_rows(self.cls_row, out=x[b, 0:1])  # class_embedding + position_embedding[0] (precomputed constant)
        x = self.pre_ln(x.view(B * T, c.hidden), out_f32=True)
        norm, lin_in, lin_out = Llama._PREFILL_FLAGS[self.precision]  # (the operands of a LLaMA prefill layer in the same mode)
        split = self.precision == "parity"
        for L in self.layers:
            if self.fp8:  # e4m3 operands for qkv / out / fc1 / fc2 (attention stays bf16, the residual stream fp32)
                sc = L["s"]
                a = self._attention(ops.linear_fp8(L["ln1"](x, fp8_scale=sc["y1"]), L["qkv_q"], sc["y1"], L["qkv_s"], L["qkv_b"]), B)
                aq = ops.gather_rows(a, out_kind="fp8", scale=sc["a"])
                x = ops.linear_fp8(aq, L["out_q"], sc["a"], L["out_s"], L["out"].b, residual=x, out_kind="f32")
                h8 = ops.linear_fp8(L["ln2"](x, fp8_scale=sc["y2"]), L["fc1_q"], sc["y2"], L["fc1_s"], L["fc1"].b, act="quick_gelu",
                                    out_kind="fp8", scale_out=sc["h"])
                x = ops.linear_fp8(h8, L["fc2_q"], sc["h"], L["fc2_s"], L["fc2"].b, residual=x, out_kind="f32")
                continue
            wq, wo, w1, w2 = (tuple(self._f16(L)[n + "_h"] for n in ("qkv", "out", "fc1", "fc2")) if self.precision == "f16"
                              else (L["qkv_w"], L["out"].w, L["fc1"].w, L["fc2"].w))
            y = L["ln1"](x, **norm)
            a = self._attention(ops.linear(y, wq, L["qkv_b"], **lin_in), B, split)
            x = ops.linear(a, wo, L["out"].b, residual=x, out_f32=True, **lin_out)
            y2 = L["ln2"](x, **norm)
            h = ops.linear(y2, w1, L["fc1"].b, act="quick_gelu", **lin_in)
            cal = L.get("amax") if self._calibrating and self.precision == "default" else None  # (enable_fp8)
            if cal:
                for k_, t_ in (("y1", y), ("a", a), ("y2", y2), ("h", h)):
                    ops.amax(t_, cal[k_])
            x = ops.linear(h, w2, L["fc2"].b, residual=x, out_f32=True, **lin_out)
        if B not in self._patch_rows:  # drop the CLS row of every image
            r = torch.arange(B * T, dtype=torch.int32).view(B, T)[:, 1:].reshape(-1)
            self._patch_rows[B] = r.to(images.device)
        # (the mm_projector takes hi + lo rows in the "parity" and "f16" modes: 0.03 % of the image's FLOPs)
        kind = "bf16" if self.precision == "default" else "split"
        return ops.gather_rows(x, self._patch_rows[B], out_kind=kind).view(B, T - 1, -1)


class _LayerW(dict):
    """One LLaMA layer's tensors: ln1 / ln2, the four bf16 matrices (qkv, o, gu, down) and their derived copies (``*_h``: IEEE fp16
    for the fp16-operand prefill, ``*_p``: ops.PackedBf12 planes for the decode step).  A bf16 matrix that ``Llama.release_unused``
    dropped comes back on access, bit for bit, from its packed planes (``ivlm_unpack_bf12``: the 12-bit format is lossless)."""

    MATS = ("qkv", "o", "gu", "down")

    def __missing__(self, k):
        p = dict.get(self, k + "_p") if k in self.MATS else None
        if p is None:
            raise KeyError(k)
        w = p.unpack().contiguous()
        self[k] = w
        return w


class Llama:
    """HF LlamaModel + lm_head with a KV cache, one sequence (batch 1) per instance call."""

    MAX_LEN_LIMIT = 4096  # the decode attention kernel keeps one score per cached position in LDS (decattn::kMaxT)

    def __init__(self, w, cfg: LlamaCfg, device, prefix="model", max_len=640):
        if max_len > self.MAX_LEN_LIMIT:
            raise ops.IvlmError(f"max_len={max_len}: the KV-cached decode kernels support at most {self.MAX_LEN_LIMIT} positions")
        self.cfg, self.device, self.max_len = cfg, device, max_len
        self.embed = _dev(w[prefix + ".embed_tokens.weight"], device)
        self.layers = []
        for i in range(cfg.layers):
            p = f"{prefix}.layers.{i}"
            qkv = torch.cat([w[f"{p}.self_attn.{n}_proj.weight"] for n in "qkv"], 0)
            gu = torch.stack([w[p + ".mlp.gate_proj.weight"], w[p + ".mlp.up_proj.weight"]], 1).reshape(
                2 * cfg.inter, cfg.hidden)  # rows (gate_j, up_j) interleaved for the SwiGLU epilogue
            self.layers.append(_LayerW(
                ln1=_dev(w[p + ".input_layernorm.weight"], device), ln2=_dev(w[p + ".post_attention_layernorm.weight"], device),
                qkv=_dev(qkv, device), o=_dev(w[p + ".self_attn.o_proj.weight"], device), gu=_dev(gu, device),
                down=_dev(w[p + ".mlp.down_proj.weight"], device)))
        self.norm = _dev(w[prefix + ".norm.weight"], device)
        self.lm_head = _dev(w["lm_head.weight"], device)
        H, hd = cfg.heads, cfg.hidden // cfg.heads
        self.kcache = torch.zeros(cfg.layers, max_len, H, hd, dtype=BF16, device=device)
        self.vcache = torch.zeros(cfg.layers, max_len, H, hd, dtype=BF16, device=device)
        self.rope = ops.rope_table(max_len, hd, cfg.theta, device)  # fp32 cos/sin, computed once
        self.precision = "default"
        self.decode_splitkv = False  # split-KV decode attention (long prompts): see _attn_scratch
        self.kcache_lo = self.vcache_lo = None  # "parity" precision: lo planes of the cache (allocated on first use)
        self._graphs = {}  # _GraphKey -> captured decode step (decode_graph / decode_graph_batch); entries leave by _drop_graphs
        self._fused = None
        # attention + o_proj in ONE launch (o_proj blocks wait on device counters): saved a launch per layer when the o_proj
        # GEMV was the persistent kernel; with gemv1_kernel the separate launches are as fast (2.67 vs 2.68 ms/token, same
        # end to end), so the simpler graph is the default and the fused launch stays opt-in (tests cover both)
        self.fuse_attn_oproj = bool(os.environ.get("IVLM_FUSE_ATTN_OPROJ"))
        # The batch-1 decode linears stream LOSSLESSLY packed weights (ops.PackedBf12: 1.5 bytes per weight, every bf16 value
        # reconstructed bit for bit, dots on the matrix cores: ivlm_gemv1_bf12m; copies made on the first decode step, +10 GB for
        # 7B): 2.69 -> 2.34 ms per token.  Matrices whose shape the fragment layout does not take (rows % 16, columns % 64) stay
        # on the bf16 kernel (the lm_head's rows are padded with zeros).  IVLM_DECODE_PACKED=0 / decode_packed = False: bf16 weights everywhere.
        self.decode_packed = os.environ.get("IVLM_DECODE_PACKED", "1") != "0"
        self.decode_attn_parts = os.environ.get("IVLM_DECODE_ATTN_PARTS", "1") != "0"  # (with decode_packed: see _decode_step)
        self.decode_packed_batch = os.environ.get("IVLM_DECODE_PACKED_BATCH", "1") != "0"  # (the batched step: ivlm_gemv16_bf12m)

    # ---- which copies of the layer matrices are resident -----------------------------------------
    # Three forms exist: the checkpoint's bf16 matrices (prefill of the bf16 / parity modes, bf16 decode), IEEE fp16 copies (prefill
    # of the fp16-operand default mode), lossless 12-bit planes (the decode step of every mode).  ``prepare`` builds, NOW, what the
    # active mode reads - so that an out-of-memory or an out-of-fp16-range weight surfaces at load / mode switch and not inside the
    # first forward; ``release_unused`` drops what it does not read: in the default mode the bf16 originals of every matrix that
    # has planes (13.5 GB for 7B; `_LayerW` rebuilds one bit for bit from its planes if a non-default path asks for it), in the
    # other modes the fp16 copies.  InteractVLMForCausalLM.set_precision calls both.
    def prepare(self):
        if self.fp8 or self._calibrating:
            return
        for L in self.layers:
            if self.decode_packed:
                for n in _LayerW.MATS:
                    self._planes(L, n)
            if self.precision == "f16":
                self._f16w(L)
            else:  # bf16 / parity prefill reads the bf16 matrices (rebuilt from the planes if the default mode had released them)
                for n in _LayerW.MATS:
                    L[n]
        if self.decode_packed and ops.PackedBf12.takes(16, self.cfg.hidden) and getattr(self, "lm_head_p", None) is None:
            self.lm_head_p = ops.PackedBf12(self.lm_head, pad_rows=True)

    def release_unused(self):
        if self.fp8 or self._calibrating:
            return
        dropped = False
        for L in self.layers:
            for n in _LayerW.MATS:
                if self.precision == "f16":
                    wp = L.get(n + "_p")
                    have16 = n + "_h" in L or n + "_hp" in L
                    if self.decode_packed and wp is not None and wp.frag and dict.__contains__(L, n) and have16:
                        del L[n]
                        dropped = True
                    if n + "_hp" in L and L.pop(n + "_h", None) is not None:  # (the panels replace the row-major copy)
                        dropped = True
                else:
                    for k in (n + "_h", n + "_hp"):
                        if L.pop(k, None) is not None:
                            dropped = True
        if dropped:  # graphs that read the bf16 matrices (unpacked steps, the fused attention + o_proj) hold pointers into them
            self._drop_graphs(lambda k: not k.packed or k.fused)

    def resident_bytes(self):
        """{form: bytes} of the language model's weights currently in HBM."""
        out = {"bf16": self.embed.numel() * 2 + self.lm_head.numel() * 2 + self.norm.numel() * 2, "f16": 0, "bf12": 0}
        for L in self.layers:
            out["bf16"] += (L["ln1"].numel() + L["ln2"].numel()) * 2
            for n in _LayerW.MATS:
                if dict.__contains__(L, n):
                    out["bf16"] += L[n].numel() * 2
                for k in (n + "_h", n + "_hp"):
                    if L.get(k) is not None:
                        out["f16"] += L[k].numel() * 2
                if L.get(n + "_p") is not None:
                    out["bf12"] += L[n + "_p"].bytes()
        if getattr(self, "lm_head_p", None) is not None:
            out["bf12"] += self.lm_head_p.bytes()
        return out

    # ---- "parity" precision (opt-in): the prefill GEMMs take hi + lo bf16 activation operands, the attention three MFMAs per
    # fragment, and K / V are cached as hi + lo planes (also read by the decode kernels) - no activation is rounded to bf16.
    # "f16": the prefill GEMMs and attention take IEEE fp16 operands (one MFMA pass, an eighth of the bf16 operand rounding; fp16
    # copies of the layer weights, +12.6 GB for 7B, made on first use), K / V are cached as fp16 (the same cache storage, seen
    # as fp16) and read as fp16 by the decode kernels, whose activations are fp32 in every mode.
    def set_precision(self, mode):
        assert mode in ("default", "parity", "f16")
        if mode == self.precision:
            return
        self.precision = mode
        if mode == "parity" and self.kcache_lo is None:
            self.kcache_lo, self.vcache_lo = torch.zeros_like(self.kcache), torch.zeros_like(self.vcache)

    # ---- fp8 (OCP e4m3; BASELINE.json configs[4], opt-in) -------------------------------------------------------------------
    # Prefill: e4m3 operands for the four GEMMs of a layer on the MX matrix instruction (per-tensor scales: weights quantised
    # once, activation ranges calibrated on one bf16 pass over a calibration prompt, then fixed; RMSNorm / SwiGLU epilogue write
    # e4m3 directly).  Decode (batch 1): e4m3 WEIGHTS, fp32 activations - the step is HBM-bound on the weight bytes, so this
    # halves its traffic (the products are exact; the only error is the weight quantisation).  lm_head, attention and the KV
    # cache stay bf16; the batched decode (evaluate_batch) keeps bf16 weights.
    fp8 = False
    _calibrating = False

    def enable_fp8(self, calib_x):
        """calib_x fp32 [T, hidden]: input embeddings of a calibration prompt (with its image features spliced in)."""
        dev = self.device
        for L in self.layers:
            for n in ("qkv", "o", "gu", "down"):
                L[n + "_q"], L[n + "_s"] = ops.quantize_fp8(L[n])
            L["amax"] = {k: torch.zeros(1, dtype=F32, device=dev) for k in ("y1", "a", "y2", "h")}
        self._calibrating = True
        try:
            self.forward(calib_x, 0)
        finally:
            self._calibrating = False
        for L in self.layers:
            L["s"] = {k: (v / 448.0).clamp_(min=1e-12) for k, v in L["amax"].items()}
        self.fp8 = True
        self._drop_graphs(lambda k: True)

    def disable_fp8(self):
        self.fp8 = False
        self._drop_graphs(lambda k: True)

    def _lo(self, li):
        return (self.kcache_lo[li], self.vcache_lo[li]) if self.precision == "parity" else None

    def _caches(self):
        """this instance's single-sequence cache in the element type of the precision mode (fp16 mode: the same bytes as fp16)"""
        if self.precision == "f16":
            return self.kcache.view(torch.float16), self.vcache.view(torch.float16)
        return self.kcache, self.vcache

    def _f16(self, L):
        """row-major fp16 copies ``*_h`` of the four matrices (the C sequencers' layout; rebuilt from bf16 if they were released)"""
        for n in _LayerW.MATS:
            if n + "_h" not in L:
                L[n + "_h"] = ops.f16_weight(L[n], "llama " + n)
        return L

    # K-panel layout of the fp16 prefill copies: [K / 64, N, 64] instead of [N, K] - the same bytes, a wave's
    # DMA instruction reads 1 KB contiguous.  The prefill GEMMs (M = 330) are bound by each CU's L1 fill path
    # (profiles/r05_gemm_ceilings.txt), which serves contiguous kilobytes faster than eight lines a row stride apart.
    prefill_panels = os.environ.get("IVLM_PREFILL_PANELS", "1") != "0"

    def _f16w(self, L):
        """-> {n: the fp16 weight the Python prefill passes to ops.linear} (panels when ``prefill_panels``, else row-major)"""
        if not self.prefill_panels or self.cfg.hidden % 64 or self.cfg.inter % 64:
            self._f16(L)
            return {n: L[n + "_h"] for n in _LayerW.MATS}
        for n in _LayerW.MATS:
            if n + "_hp" not in L:
                h = L.pop(n + "_h") if n + "_h" in L else ops.f16_weight(L[n], "llama " + n)
                L[n + "_hp"] = ops.panel_weight(h)  # (the row-major copy is not kept: _f16 rebuilds it for the C sequencers)
        return {n: L[n + "_hp"] for n in _LayerW.MATS}

    def batch_cache_lo(self, B):
        bc = getattr(self, "_bcache_lo", None)
        if bc is None or bc[0].shape[1] < B:
            kc, vc = self.batch_cache(B)
            bc = self._bcache_lo = (torch.zeros_like(self._bcache[0]), torch.zeros_like(self._bcache[1]))
            self._drop_graphs(lambda k: k.batched and k.precision == "parity")
        return bc[0][:, :B], bc[1][:, :B]

    def embed_ids(self, ids_i32, out=None):
        """embed_tokens gather: ids int32 [n] -> fp32 [n, hidden] (the start of the fp32 residual stream)."""
        return ops.gather_rows(self.embed, ids_i32, out=out, out_kind="f32")

    def forward(self, x, pos0, cache=None):
        """x fp32 [T, hidden] input embeddings at positions pos0..pos0+T-1 -> final-norm hidden fp32 [T, hidden];
        appends to the KV cache (prefill: T = prompt, decode: T = 1).  cache = (k, v[, k_lo, v_lo]) [layers, Tmax, H, hd] views
        of another sequence's slab (batched generation); default: this instance's single-sequence cache."""
        T = x.shape[0]
        assert pos0 + T <= self.max_len and x.dtype == F32
        if T == 1 and cache is None:
            return self._decode_step(x, pos0)
        if 1 < T <= 16 and cache is None and self.precision != "default":
            # (the fp16 / split tile GEMMs need M > 16: a short chunk goes token by token through the fp32-activation decode
            #  kernels, which are exact on the bf16 weights)
            return torch.cat([self._decode_step(x[t: t + 1], pos0 + t) for t in range(T)], 0)
        if cache is None:
            cache = self._caches() + ((self.kcache_lo, self.vcache_lo) if self.precision == "parity" else ())
        return self._prefill(x, [(0, T, pos0, cache)])[0]

    def forward_packed(self, xs, kc, vc, lo=None):
        """Prefill of B sequences in ONE pass over the weights: xs = [x_b fp32 [T_b, hidden]] (lengths may differ), kc / vc
        [layers, B, Tmax, H, hd] cache slabs (lo = their (k_lo, v_lo) slabs in "parity") -> [final-norm hidden fp32 [T_b, hidden]].
        Row-wise identical arithmetic to ``forward``: B = 1 is forward(xs[0], 0, cache=slab 0)."""
        assert max(int(x.shape[0]) for x in xs) <= self.max_len
        segs, r0 = [], 0
        for b, x in enumerate(xs):
            segs.append((r0, r0 + x.shape[0], 0, (kc[:, b], vc[:, b]) + ((lo[0][:, b], lo[1][:, b]) if lo is not None else ())))
            r0 += x.shape[0]
        return self._prefill(torch.cat(xs, 0) if len(xs) > 1 else xs[0], segs)  # (one sequence: its rows as they are, no copy)

    # ---- several prompts about ONE picture: the leading P spliced positions (system text + image features) are the same rows in
    # every sequence.  They are prefilled ONCE (into slab 0) and copied to the other slabs - every slab ends up complete, so the
    # plain batched decode kernel stays valid on the same state -, then the B suffixes run as packed segments that start at
    # position P.  P comes from decoding.shared_prefix_len; not in the "parity" mode or with fp8 (as verify_step).
    def prefix_supported(self):
        return self.precision != "parity" and not self.fp8

    def forward_shared_prefix(self, xs, P, kc, vc):
        """forward_packed for B >= 2 sequences whose first P rows are identical: xs = [x_b fp32 [T_b, hidden]], P > 16 and
        P < min(T_b), more than 16 suffix rows in all (the tile GEMMs need M > 16) -> [final-norm hidden fp32 [T_b, hidden]]."""
        B = len(xs)
        T = [int(x.shape[0]) for x in xs]
        if not self.prefix_supported():
            raise ops.IvlmError(f"forward_shared_prefix: not in precision {self.precision!r} / fp8")
        if B < 2 or not 16 < P < min(T) or sum(T) - B * P <= 16 or max(T) > self.max_len:
            raise ops.IvlmError(f"forward_shared_prefix: B={B}, P={P}, lengths {T}: need B >= 2, 16 < P < min length, > 16 suffix rows")
        pre = self._prefill(xs[0][:P], [(0, P, 0, (kc[:, 0], vc[:, 0]))])[0]
        for c in (kc, vc):  # one broadcast copy per cache: rows [0, P) of slab 0 -> slabs 1 .. B-1, every layer
            c[:, 1:, :P].copy_(c[:, :1, :P])
        segs, r0 = [], 0
        for b in range(B):
            segs.append((r0, r0 + T[b] - P, P, (kc[:, b], vc[:, b])))
            r0 += T[b] - P
        suf = self._prefill(torch.cat([x[P:] for x in xs], 0), segs)
        return [torch.cat([pre, h], 0) for h in suf]

    def _prefill(self, x, segs):
        """The prefill layers on the packed rows x fp32 [rows, hidden] of one or more sequences; segs = [(r0, r1, pos0, cache)]: a
        sequence's rows, the position of its first row and its cache planes (k, v[, k_lo, v_lo]) [layers, Tmax, H, hd]
        -> [final-norm hidden fp32 [r1 - r0, hidden]] per sequence.  The four projections of a layer run on all rows (M = sum of
        the lengths: one efficient GEMM instead of B skinny ones, weights streamed once); RoPE + cache append and the causal
        attention run per sequence.  The residual stream is fp32 (GEMM residual epilogues write fp32, RMSNorm reads it).
        fp8 operands (enable_fp8) for one sequence of more than 16 rows only, never while calibrating."""
        fp8 = self.fp8 and not self._calibrating and len(segs) == 1 and x.shape[0] > 16
        for li in range(len(self.layers)):
            x = self._prefill_layer(li, x, segs, fp8)
        x = ops.rmsnorm(x, self.norm, self.cfg.eps, out_f32=True)
        return [x[r0: r1] for r0, r1, _, _ in segs]

    # the MFMA operands of a prefill layer per precision mode: the rmsnorm flags, the flags of the q|k|v and gate|up GEMMs (whose
    # outputs are operands again) and those of the o and down GEMMs (fp32 residual out).  "default": bf16; "f16": IEEE fp16 (the
    # _f16w copies of the weights); "parity": [hi | lo] bf16 rows (fp32 activations) on the bf16 weights
    _PREFILL_FLAGS = {"default": ({}, {}, {}),
                      "f16": (dict(out_f16=True), dict(out_f16=True), {}),
                      "parity": (dict(out_split=True), dict(a_split=True, out_split=True), dict(a_split=True))}

    def _prefill_layer(self, li, x, segs, fp8=False):
        """prefill layer li on the packed rows x fp32 [rows, hidden] of segs (see _prefill) -> fp32 [rows, hidden]"""
        c, L = self.cfg, self.layers[li]
        if fp8:  # e4m3 operands with the calibrated per-tensor scales; attention stays bf16
            sc = L["s"]
            qkv = ops.linear_fp8(ops.rmsnorm(x, L["ln1"], c.eps, fp8_scale=sc["y1"]), L["qkv_q"], sc["y1"], L["qkv_s"])
            a8 = ops.gather_rows(self._prefill_attn(qkv, li, segs), out_kind="fp8", scale=sc["a"])
            x = ops.linear_fp8(a8, L["o_q"], sc["a"], L["o_s"], residual=x, out_kind="f32")
            h8 = ops.linear_fp8(ops.rmsnorm(x, L["ln2"], c.eps, fp8_scale=sc["y2"]), L["gu_q"], sc["y2"], L["gu_s"], act="swiglu",
                                out_kind="fp8", scale_out=sc["h"])
            return ops.linear_fp8(h8, L["down_q"], sc["h"], L["down_s"], residual=x, out_kind="f32")
        norm, lin_in, lin_out = self._PREFILL_FLAGS[self.precision]
        W = self._f16w(L) if self.precision == "f16" else L
        y = ops.rmsnorm(x, L["ln1"], c.eps, **norm)
        a = self._prefill_attn(ops.linear(y, W["qkv"], **lin_in), li, segs)
        x = ops.linear(a, W["o"], residual=x, out_f32=True, **lin_out)
        y2 = ops.rmsnorm(x, L["ln2"], c.eps, **norm)
        h = ops.linear(y2, W["gu"], act="swiglu", **lin_in)
        if self._calibrating and self.precision == "default":  # the activation ranges of the fp8 operands (enable_fp8)
            for k, t in (("y1", y), ("a", a), ("y2", y2), ("h", h)):
                ops.amax(t, L["amax"][k])
        return ops.linear(h, W["down"], residual=x, out_f32=True, **lin_out)

    def _prefill_attn(self, qkv, li, segs):
        """RoPE + cache append + causal attention of layer li, sequence by sequence: qkv [rows, 3*hidden] ("parity": [hi | lo]
        rows [rows, 6*hidden]) -> the attention rows [rows, hidden] in qkv's dtype ("parity": [rows, 2*hidden] = [hi | lo])"""
        c = self.cfg
        H, hd = c.heads, c.hidden // c.heads
        a = torch.empty(qkv.shape[0], qkv.shape[1] // 3, dtype=qkv.dtype, device=qkv.device)
        for r0, r1, pos0, cache in segs:
            T, qs, out = r1 - r0, qkv[r0: r1], a[r0: r1]
            if self.precision == "parity":
                kc, vc, kcl, vcl = (t[li] for t in cache)
                ops.rope_kv_split(qs, H, hd, pos0, (kc, kcl, vc, vcl), self.rope)
                qh, ql = (qs.view(T, 2, 3, H, hd)[:, i, 0].permute(1, 0, 2).unsqueeze(0) for i in range(2))
                kv = [t[: pos0 + T].permute(1, 0, 2).unsqueeze(0) for t in (kc, kcl, vc, vcl)]
                ops.attention_split(qh, ql, *kv, hd ** -0.5, causal=True, q_pos0=pos0, out=out.view(1, T, 2, H, hd))
            else:
                kc, vc = cache[0][li], cache[1][li]
                ops.rope_kv(qs, H, hd, pos0, c.theta, kc, vc, table=self.rope)
                q = qs.view(T, 3, H, hd)[:, 0].permute(1, 0, 2).unsqueeze(0)  # [1, H, T, hd]
                k, v = (t[: pos0 + T].permute(1, 0, 2).unsqueeze(0) for t in (kc, vc))
                ops.attention(q, k, v, hd ** -0.5, causal=True, q_pos0=pos0, out=out.view(1, T, H, hd).permute(0, 2, 1, 3))
        return a

    # ---- one decode step as a replayable HIP graph ------------------------------------------------------------------
    # Static buffers: token id in, position (device int32, read by the attention kernel), hidden out, argmax out.
    # Per generated token the host then issues 1 graph launch instead of ~165 kernel launches (2.4 ms of Python).
    # The graphs are cached per _GraphKey: switching precision or `decode_packed` selects another entry, and whatever frees or
    # replaces a buffer that a captured step reads (weights, cache slabs) drops the entries that read it (_drop_graphs).
    def _graph_key(self, B, batched):
        if batched:
            return _GraphKey(True, B, self.precision, self.decode_packed and self.decode_packed_batch and B > 1, self.fp8, False)
        c = self.cfg
        # (every block of the fused launch must be resident at once: one 1024-thread block per CU; hidden % heads == 0, as everywhere here)
        fused = bool(self.fuse_attn_oproj and _lib.load().ivlm_llama_attn_oproj_fits(
            c.heads, c.hidden // c.heads, torch.cuda.get_device_properties(self.device).multi_processor_count))
        return _GraphKey(False, 1, self.precision, bool(self.decode_packed), self.fp8, fused)

    def _drop_graphs(self, pred):
        """the only way a captured decode step leaves the cache: called where a buffer it may have baked in is freed or replaced"""
        self._graphs = {k: st for k, st in self._graphs.items() if not pred(k)}

    def fused_wait_expired(self, st):
        """after the replays of decode_graph state st: did a bounded device-side wait of the fused attention + o_proj launch expire
        (its blocks were not co-resident, e.g. a third stream holding the CUs)?  Then the fused steps are dropped and the two-launch
        path is used for good: the caller redoes the generation."""
        fz = st.get("fused")
        if fz is None or int(fz["status"].item()) == 0:
            return False
        self.fuse_attn_oproj = False
        self._drop_graphs(lambda k: k.fused)
        return True

    def _capture_decode(self, key, st, body, caches, counters, rows=1):
        """capture body (one decode step) into st["graph"] and cache st under key.  The warm-up run writes KV rows 0 .. rows-1 of
        every cache plane and advances the counters (positions, fused-launch counters): both are put back."""
        saved = [t[..., :rows, :, :].clone() for t in caches]  # (fp16 mode: the same bytes)
        st["graph"], _ = graphs.capture(body, self.device)
        for t in counters:
            t.zero_()
        for t, sv in zip(caches, saved):
            t[..., :rows, :, :].copy_(sv)
        self._graphs[key] = st

    def decode_graph(self, pos=None):
        """the captured batch-1 step; pos: a generation starts at this position (resets the position and the fused-launch counters)"""
        key = self._graph_key(1, batched=False)
        st = self._graphs.get(key)
        if st is None:
            dev, c = self.device, self.cfg
            st = dict(tok=torch.zeros(1, dtype=torch.int32, device=dev), pos=torch.zeros(1, dtype=torch.int32, device=dev),
                      pos64=torch.zeros(1, dtype=torch.int64, device=dev))
            if key.fused:
                # fused attention + o_proj launches: per-layer arrival counters, tokens-decoded counter, status word
                st["fused"] = dict(step=torch.zeros(1, dtype=torch.int32, device=dev),
                                   counters=torch.zeros(c.layers, 32, dtype=torch.int32, device=dev),  # 128-B apart
                                   status=torch.zeros(1, dtype=torch.int32, device=dev),
                                   scratch=torch.zeros(c.layers, c.hidden, dtype=F32, device=dev))
            fz = self._fused = st.get("fused")

            def body():
                e = self.embed_ids(st["tok"])
                h = self._decode_step(e, st["pos"])
                st["hidden"] = h
                st["nxt"] = ops.argmax(self.logits(h), bump=st["pos"])  # (+ position += 1 in the same launch)
                if fz is not None:
                    fz["step"].add_(1)

            caches = [self.kcache, self.vcache] + ([self.kcache_lo, self.vcache_lo] if self.precision == "parity" else [])
            counters = [st["pos"], st["pos64"]] + ([fz["step"], fz["counters"]] if fz is not None else [])
            self._capture_decode(key, st, body, caches, counters)
        if pos is not None:
            st["pos"].fill_(pos)
            st["pos64"].fill_(pos)
            if "fused" in st:
                for k in ("step", "counters", "status"):
                    st["fused"][k].zero_()
        return st

    # ---- B sequences per decode step (configs[2]: 8 images per GPU) ---------------------------------------------------
    # The weights are streamed once per step for all B tokens (GEMV rows M = B <= 8 share every weight load), so a step of
    # 8 sequences costs little more than a step of one.  Each sequence owns a cache slab [Tmax, H, hd] per layer.
    def batch_cache(self, B):
        bc = getattr(self, "_bcache", None)
        if bc is None or bc[0].shape[1] < B:
            c = self.cfg
            H, hd = c.heads, c.hidden // c.heads
            bc = self._bcache = tuple(torch.zeros(c.layers, B, self.max_len, H, hd, dtype=BF16, device=self.device)
                                      for _ in range(2))
            self._drop_graphs(lambda k: k.batched)
        if self.precision == "f16":  # the same slabs, seen as fp16
            return bc[0].view(torch.float16)[:, :B], bc[1].view(torch.float16)[:, :B]
        return bc[0][:, :B], bc[1][:, :B]

    def decode_step_batch(self, x, pos_dev, kc, vc, lo=None, prefix=None):
        """x fp32 [B, hidden] (one new token per sequence), pos_dev int32 [B], kc/vc [layers, B, Tmax, H, hd] ->
        final-norm hidden fp32 [B, hidden]; same arithmetic per row as ``_decode_step`` (fp32 activations: the skinny MFMA
        kernel splits them into hi + lo bf16 operands, the batch-1 GEMV multiplies them exactly - equal to ~1e-5).
        prefix (int32 [1] on the device, or None): the first prefix[0] cached rows are the same in every slab
        (forward_shared_prefix) and the attention reads them from slab 0 once for all sequences (ops.llama_decode_attn_batch_prefix)."""
        c = self.cfg
        H, hd = c.heads, c.hidden // c.heads
        if x.shape[0] > 16:
            raise ops.IvlmError("decode_step_batch: at most 16 sequences per step (weight-streaming kernels)")
        lin = self._lin("frag" if self.decode_packed and self.decode_packed_batch and x.shape[0] > 1 else None)
        if prefix is not None:
            if lo is not None or not self.prefix_supported():
                raise ops.IvlmError(f"decode_step_batch(prefix=...): not in precision {self.precision!r} / fp8")
            if getattr(self, "_prefix_scratch", None) is None:  # (sized for 16 sequences: one buffer for every B)
                self._prefix_scratch = ops.decode_attn_prefix_scratch(16, H, hd, self.norm.device)
            return self._decode_layers(x, lin, self._attn_then_o(lin, lambda qkv, li: (
                ops.llama_decode_attn_batch_prefix(qkv, kc[li], vc[li], H, hd, pos_dev, prefix, c.theta, hd ** -0.5, table=self.rope,
                                                   scratch=self._prefix_scratch))))
        return self._decode_layers(x, lin, self._attn_then_o(lin, lambda qkv, li: (
            ops.llama_decode_attn_batch(qkv, kc[li], vc[li], H, hd, pos_dev, c.theta, hd ** -0.5, table=self.rope,
                                        lo=(lo[0][li], lo[1][li]) if lo is not None else None))))

    @staticmethod
    def _planes(L, n):
        """the lossless 12-bit decode planes of matrix n of layer L (ops.PackedBf12), made on first use; None where the fragment
        layout does not take the matrix's shape"""
        if n + "_p" not in L:
            L[n + "_p"] = ops.PackedBf12(L[n]) if ops.PackedBf12.takes(*L[n].shape) else None
        return L[n + "_p"]

    def _decode_layers(self, x, lin, attn_o):
        """the layers of every decode step (_decode_step, decode_step_batch, verify_step): x fp32 [rows, hidden] -> final-norm
        hidden fp32.  lin(x, L, name, **kw): the linear of matrix name of layer L on fp32 rows (which weights, which kernel);
        attn_o(qkv, li, L, x) -> the residual stream after the attention and o_proj of layer li (separate or merged launches)"""
        c = self.cfg
        for li, L in enumerate(self.layers):
            qkv = lin(x, L, "qkv", rms=(L["ln1"], c.eps))
            x = attn_o(qkv, li, L, x)
            h = lin(x, L, "gu", act="swiglu", rms=(L["ln2"], c.eps))
            x = lin(h, L, "down", residual=x)
        return ops.rmsnorm(x, self.norm, c.eps, out_f32=True)

    @staticmethod
    def _attn_then_o(lin, attn):
        """the attn_o of _decode_layers from attn(qkv, li) -> the attention rows of layer li: then o_proj + residual through lin"""
        return lambda qkv, li, L, x: lin(attn(qkv, li), L, "o", residual=x)

    def _lin(self, planes=None):
        """a lin of _decode_layers on the bf16 weights: the 12-bit planes (_planes) where planes = "any" (batch 1: every matrix that
        has them) or "frag" (several rows: the fragment layout only; the weights streamed once for all rows), the bf16 matrix
        otherwise"""
        def lin(x, L, n, **kw):
            wp = self._planes(L, n) if planes else None
            if wp is not None and (planes == "any" or wp.frag):
                return ops.linear_bf12(x, wp, **kw)
            return ops.linear(x, L[n], out_f32=True, **kw)
        return lin

    # ---- speculative greedy decoding: k <= 16 new tokens of THIS instance's sequence in one pass over the weights -----------------
    # The rows [t0, d1 .. d_{k-1}] (last emitted token + a draft) sit at positions pos .. pos+k-1 of the single-sequence cache; one
    # pass costs about what a batched step of k sequences costs (the linears of decode_step_batch), and an accepted draft token saves a
    # whole decode step.  Not in the "parity" mode (hi + lo cache planes) or with fp8 weights: the generation loop runs the plain
    # step there (InteractVLMForCausalLM.generate).
    VERIFY_BUCKETS = (4, 8, 16)  # rows per captured verify pass (a shorter draft is padded; padded rows are never accepted)

    def verify_supported(self):
        return self.precision != "parity" and not self.fp8

    def verify_step(self, x, pos_dev):
        """x fp32 [k, hidden] (k <= 16 new tokens), pos_dev int32 [1] = position of row 0 on the device -> final-norm hidden fp32
        [k, hidden]; appends k rows to the cache (rows at or past max_len are not appended).  Row i equals the i-th of k sequential
        ``_decode_step`` calls to the batch-vs-single tolerance of decode_step_batch (the same linears), the cache rows bit for bit."""
        c = self.cfg
        H, hd = c.heads, c.hidden // c.heads
        if not 1 <= x.shape[0] <= 16:
            raise ops.IvlmError("verify_step: 1 .. 16 rows per pass (weight-streaming kernels)")
        if not self.verify_supported():
            raise ops.IvlmError(f"verify_step: not in precision {self.precision!r} / fp8 (no multi-token attention on hi + lo planes)")
        kc, vc = self._caches()
        lin = self._lin("frag" if self.decode_packed and self.decode_packed_batch else None)
        return self._decode_layers(x, lin, self._attn_then_o(lin, lambda qkv, li: (
            ops.llama_verify_attn(qkv, kc[li], vc[li], H, hd, pos_dev, c.theta, hd ** -0.5, table=self.rope))))

    def verify_pass(self, st):
        """embed st["ids"] -> verify_step -> lm_head -> argmax -> accept (st: the static buffers of verify_graph)"""
        h = self.verify_step(self.embed_ids(st["ids"]), st["pos"])
        st["hidden"] = h
        st["amax"] = ops.argmax(self.logits(h))
        ops.spec_accept(st["amax"], st["ids"], st["nd"], st["n_acc"], st["tok"], st["pos"])
        return st

    def verify_state(self, kb):
        """fresh static buffers of a verify pass of kb rows: ids fed, draft length, position (advanced by the accept step), accepted
        count, next token"""
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=self.device)
        return dict(ids=i32(kb), nd=i32(1), pos=i32(1), n_acc=i32(1), tok=i32(1))

    def verify_graph(self, kb):
        """the verify pass of kb rows (one of VERIFY_BUCKETS) as a HIP graph; cached and dropped with the decode steps (_drop_graphs)"""
        key = _GraphKey(False, kb, self.precision, bool(self.decode_packed and self.decode_packed_batch), self.fp8, False, True)
        st = self._graphs.get(key)
        if st is None:
            st = self.verify_state(kb)
            caches = [self.kcache, self.vcache]
            self._capture_decode(key, st, lambda: self.verify_pass(st), caches, [st["pos"], st["n_acc"], st["tok"]], rows=kb)
        return st

    def decode_graph_batch(self, B, pos=None, prefix=None):
        """One batched decode step (embed -> layers -> norm -> lm_head -> argmax, positions += 1) as a HIP graph; pos (int32 [B] on
        the device): a generation starts at these positions.  prefix (host int P, or None): the shared-prefix variant of the step
        (decode_step_batch(prefix=...)), captured under its own key; P is written to device memory, so one graph serves every P."""
        kc, vc = self.batch_cache(B)
        lo = self.batch_cache_lo(B) if self.precision == "parity" else None
        key = self._graph_key(B, batched=True)
        if prefix is not None:
            key = key._replace(prefix=True)
        st = self._graphs.get(key)
        if st is None:
            dev = self.device
            st = dict(tok=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev))
            if prefix is not None:
                st["prefix"] = torch.zeros(1, dtype=torch.int32, device=dev)

            def body():
                h = self.decode_step_batch(self.embed_ids(st["tok"]), st["pos"], kc, vc, lo, st.get("prefix"))
                st["hidden"] = h
                st["nxt"] = ops.argmax(self.logits(h), bump=st["pos"])  # (+ positions += 1 in the same launch)

            self._capture_decode(key, st, body, [kc, vc] + list(lo or ()), [st["pos"]])
        if pos is not None:
            st["pos"].copy_(pos)
        if prefix is not None:
            st["prefix"].fill_(int(prefix))
        return st

    def _attn_scratch(self):
        """Scratch of the split-KV decode attention, or None = the one-block-per-head kernel.  Opt-in (`decode_splitkv = True` before
        the first decode step, or IVLM_DECODE_SPLITKV=1): measured on the 7B shapes it is even at 330 cached positions (the headline
        prompt: 2.72 vs 2.70 ms/token) and ahead from ~450 (640 positions: 2.79 vs 2.91 ms/token)."""
        if not (self.decode_splitkv or os.environ.get("IVLM_DECODE_SPLITKV", "0") == "1") or self.precision == "parity":
            return None
        if getattr(self, "_dec_scratch", None) is None:
            self._dec_scratch = ops.decode_attn_scratch(self.cfg.heads, self.cfg.hidden // self.cfg.heads, self.norm.device)
        return self._dec_scratch

    def _decode_step(self, x, pos):
        """One new token, x fp32 [1, hidden]: 4 launches per layer (RMSNorm fused into the q|k|v and gate|up GEMVs, RoPE +
        cache append + attention + o_proj + residual in one launch, SwiGLU and the other residual add in GEMV epilogues).
        Every activation between the weight-streaming kernels is fp32 and the bf16-weight x fp32-activation products are
        exact: no operand rounding on the decode path (it is HBM-bound; the fp32 traffic is a few hundred KB per token)."""
        c = self.cfg
        H, hd = c.heads, c.hidden // c.heads
        fz = self._fused if isinstance(pos, torch.Tensor) else None
        if self.fp8:  # e4m3 weights, fp32 activations: half the bytes per token (on the bf16 cache)
            lin = lambda x_, L, n, **kw: ops.linear_fp8w(x_, L[n + "_q"], L[n + "_s"], **kw)
            return self._decode_layers(x, lin, self._attn_then_o(lin, lambda qkv, li: ops.llama_decode_attn(
                qkv, self.kcache[li], self.vcache[li], H, hd, pos, c.theta, hd ** -0.5, table=self.rope)))
        kc, vc = self._caches()
        packed = self.decode_packed and fz is None  # (a fused step streams the bf16 weights)
        lin = self._lin("any" if packed else None)
        attn_o = plain = self._attn_then_o(lin, lambda qkv, li: ops.llama_decode_attn(
            qkv, kc[li], vc[li], H, hd, pos, c.theta, hd ** -0.5, table=self.rope, lo=self._lo(li), scratch=self._attn_scratch()))
        if packed:
            # attention as 4 key ranges per head whose (o, max, sum) partials the o_proj merges in its prologue (128 blocks instead of
            # 32, no merge launch): when o_proj is packed and K / V are single planes (not the hi + lo planes of "parity")
            split = self.decode_attn_parts and self._lo(0) is None
            if split and getattr(self, "_parts", None) is None:
                self._parts = torch.zeros(H * 4 * (hd + 4), dtype=F32, device=self.norm.device)

            def attn_o(qkv, li, L, x):
                wo = self._planes(L, "o")
                if not split or wo is None:
                    return plain(qkv, li, L, x)
                ops.llama_decode_attn_parts(qkv, kc[li], vc[li], H, hd, pos, c.theta, hd ** -0.5, self._parts, table=self.rope)
                return ops.linear_bf12(None, wo, residual=x, parts=(self._parts, hd))
        elif fz is not None and self.precision == "default":  # attention + o_proj + residual in one launch (W_o streams while the attention runs)
            attn_o = lambda qkv, li, L, x: ops.llama_attn_oproj(
                qkv, self.kcache[li], self.vcache[li], L["o"], x, H, hd, pos, fz["step"], fz["counters"][li], fz["status"], c.theta,
                hd ** -0.5, self.rope, fz["scratch"][li])
        return self._decode_layers(x, lin, attn_o)

    def logits(self, hidden_rows):
        """lm_head on fp32 [n, hidden] -> f32 [n, vocab].  n <= 16: exact fp32 activations on the weight-streaming kernels; more rows:
        one tile GEMM on [hi | lo] bf16 operands (fp32-equivalent activations, the weight matrix read once - ADVICE r3: 16-row
        chunks re-streamed the 262 MB of lm_head once per chunk)."""
        if hidden_rows.shape[0] > 16:
            return ops.linear(ops.split_rows(hidden_rows.contiguous()), self.lm_head, out_f32=True, a_split=True)
        if hidden_rows.shape[0] == 1 and self.decode_packed and ops.PackedBf12.takes(16, self.cfg.hidden):
            if getattr(self, "lm_head_p", None) is None:  # (the decode step's lm_head: 12-bit weights, rows padded to 16 with zeros)
                self.lm_head_p = ops.PackedBf12(self.lm_head, pad_rows=True)
            return ops.linear_bf12(hidden_rows.contiguous(), self.lm_head_p)
        return ops.linear(hidden_rows, self.lm_head, out_f32=True)
