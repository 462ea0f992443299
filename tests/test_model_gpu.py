"""GPU parity of the model stages (SAM encoder / decoder, CLIP, LLaMA, the InteractVLM facade) against the
reference-generated goldens and the fp32 CPU oracle, on synthetic weights rounded to bf16.

Precision policy of the HIP path: bf16 weights (the checkpoint's dtype), fp32 residual streams, bf16 MFMA
operands in the three big transformers (CLIP / LLaMA prefill / SAM encoder), fp32 activations with exact products on the
weight-streaming decode kernels, and an fp32-activation SAM mask decoder (hi + lo operand split).  The oracle is fp32 with
the SAME bf16-rounded weights.  Stage outputs that pass through bf16 MFMA operands are compared at ~1e-2 of their dynamic
range; the final per-vertex contact probabilities at the north star's 1e-3."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bf16_weights(spec, seed=0):
    """fp32 weights whose values are exactly bf16-representable (shared by oracle and HIP path)."""
    import torch

    from interactvlm_amd import weights as Wt

    w = Wt.synth_weights(spec, seed)
    return {k: v.to(torch.bfloat16).float() for k, v in w.items()}


# Stage bounds of the tower-level bf16-operand path (the towers' own "default"): ~1.5 x the measured figures (printed by the tests),
# so that a regression of the bf16 path cannot hide inside a loose bound
# measured (round 4): SAM small 1.48e-2 (vs the reference's fp32-WEIGHT golden: includes the checkpoint rounding), SAM blocks at
# ViT-H width 8.9e-3, CLIP 3.7e-3, LLaMA 5.5e-3 / logits 4.2e-3
BOUND_SAM_SMALL, BOUND_SAM_BLOCKS, BOUND_CLIP, BOUND_LLAMA = 2.2e-2, 1.4e-2, 6e-3, 8e-3


def _rel_err(got, ref):
    import torch

    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def test_sam_decoder_vs_reference_golden(hip_lib, cuda, golden_dir):
    """HIP prompt-encoder/mask-decoder/postprocess vs the reference's own outputs (fp32 weights there)."""
    import torch

    from interactvlm_amd import sam, synth
    from interactvlm_amd import weights as Wt

    w = Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()})
    dec = sam.SamMaskDecoder(w, cuda)
    for V in (4, 1):
        d = np.load(os.path.join(golden_dir, f"sam_decoder_V{V}.npz"))
        emb = torch.from_numpy(synth.synth_normal(f"samdec/image_emb/{V}", (V, 256, 64, 64), 1.0, 0))
        text = torch.from_numpy(synth.synth_normal(f"samdec/text/{V}", (1, V, 256), 1.0, 0))
        emb_cl = emb.permute(0, 2, 3, 1).reshape(V, 4096, 256).to(torch.bfloat16).to(cuda)
        low, iou = dec(emb_cl, text.to(torch.bfloat16).to(cuda).float())
        assert low.shape == (V, 1, 256, 256) and low.dtype == torch.float32 and iou.shape == (V, 1)
        # the call above replayed the chain as one HIP graph (configs[4]); the eager chain and a second replay with other
        # inputs in between give the same bits
        assert dec.use_graph and len(dec._graphs) >= 1
        low_e, iou_e = dec._forward(emb_cl, text.to(torch.bfloat16).to(cuda).float())
        dec(emb_cl.flip(0).contiguous(), text.to(torch.bfloat16).to(cuda).float() * 0.5)
        low_r, iou_r = dec(emb_cl, text.to(torch.bfloat16).to(cuda).float())
        assert torch.equal(low, low_e) and torch.equal(iou, iou_e) and torch.equal(low_r, low) and torch.equal(iou_r, iou)
        ref = torch.from_numpy(d["low_res"])
        assert _rel_err(low, ref) < 4e-2, _rel_err(low, ref)
        assert float((iou.cpu() - torch.from_numpy(d["iou"])).abs().max()) < 5e-2
        full = sam.postprocess_masks(low, (1024, 1024), (1024, 1024))
        assert _rel_err(full[..., ::16, ::16], torch.from_numpy(d["post_sub"])) < 4e-2
        pe = dec.key_pe.float().cpu().view(64, 64, 256).permute(2, 0, 1)[None]
        assert float((pe[..., ::8, ::8] - torch.from_numpy(d["dense_pe_sub"])).abs().max()) < 1e-4
        # against the fp32 oracle on the SAME bf16-rounded weights and inputs: the decoder keeps fp32 activations (hi + lo
        # operand split on the matrix cores, fp32 attention), so only fp32 summation-order noise is left
        from oracle import nn as O
        wb = {k: (v.to(torch.bfloat16).float() if "gaussian" not in k else v) for k, v in w.items()}
        embf, textf = emb.to(torch.bfloat16).float(), text.to(torch.bfloat16).float()
        sp_, de_ = O.prompt_encoder_text(wb, Wt.SAM_PREFIX + ".prompt_encoder", textf, (64, 64))
        pe_ = O.dense_pe(wb, Wt.SAM_PREFIX + ".prompt_encoder", (64, 64))
        low_o, iou_o = O.mask_decoder(wb, Wt.SAM_PREFIX + ".mask_decoder", embf, pe_, sp_, de_)
        e_low = float((low.cpu() - low_o).abs().max() / low_o.abs().max())
        print(f"\n[SAM decoder V={V}] vs fp32 oracle on identical weights: rel max err low_res {e_low:.2e}, "
              f"iou {float((iou.cpu() - iou_o).abs().max()):.2e}")
        assert e_low < 2e-4 and float((iou.cpu() - iou_o).abs().max()) < 2e-4


def test_sam_encoder_small_vs_reference_golden(hip_lib, cuda, golden_dir):
    import torch

    from interactvlm_amd import sam, synth
    from interactvlm_amd import weights as Wt

    d = np.load(os.path.join(golden_dir, "sam_encoder_small.npz"))
    c = Wt.SamEncCfg(embed_dim=160, depth=2, num_heads=2, global_attn_indexes=(1,), img_size=480)
    w = Wt.synth_weights(Wt.sam_encoder_spec(c))
    enc = sam.SamImageEncoder(w, c, cuda)
    x = torch.from_numpy(synth.synth_normal("samenc/x", (2, 3, 480, 480), 1.0, 0)).to(torch.bfloat16).to(cuda)
    y = enc(x)  # [2, 900, 256] channels last
    ref = torch.from_numpy(d["out"]).permute(0, 2, 3, 1).reshape(2, 900, 256)
    print(f"\n[SAM encoder small, bf16 operands vs the reference's fp32-weight output] rel err {_rel_err(y, ref):.2e}")
    assert _rel_err(y, ref) < BOUND_SAM_SMALL, _rel_err(y, ref)


def test_sam_encoder_vith_dimensions_vs_reference_golden(hip_lib, cuda, golden_dir):
    """HIP SAM encoder at the real ViT-H layer dimensions (head dim 80 padded to 96 in the MFMA attention, 14x14 windows with
    padding 64 -> 70, the global block with 127-row rel-pos tables, neck) against the reference's own output (depth 2)."""
    import torch

    from interactvlm_amd import sam, synth
    from interactvlm_amd import weights as Wt

    d = np.load(os.path.join(golden_dir, "sam_encoder_vith_dims.npz"))
    c = Wt.SamEncCfg(depth=2, global_attn_indexes=(1,))
    w = Wt.synth_weights(Wt.sam_encoder_spec(c))
    enc = sam.SamImageEncoder(w, c, cuda)
    x = torch.from_numpy(synth.synth_normal("samenc_full/x", (1, 3, 1024, 1024), 1.0, 0)).to(torch.bfloat16).to(cuda)
    y = enc(x).float().cpu().view(1, 64, 64, 256).permute(0, 3, 1, 2)  # -> [1,256,64,64]
    ref = torch.from_numpy(d["out_sub"])
    got = y[:, ::4, ::2, ::2]
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"\n[SAM ViT-H dims, depth 2] rel rms err vs reference = {rel:.4f}, max abs = {float((got - ref).abs().max()):.4f}")
    assert rel < 1.8e-2 and float((got - ref).abs().max()) < 0.1 * float(ref.abs().max())  # (measured 1.21e-2)


def test_sam_block_full_dims_vs_oracle(hip_lib, cuda):
    """One windowed + one global block at ViT-H width (1280 / 16 heads / head dim 80) on a 64x64 grid."""
    import torch

    from interactvlm_amd import sam
    from interactvlm_amd import weights as Wt
    from oracle import nn as O

    c = Wt.SamEncCfg(embed_dim=1280, depth=2, num_heads=16, global_attn_indexes=(1,), img_size=1024)
    w = _bf16_weights(Wt.sam_encoder_spec(c))
    enc = sam.SamImageEncoder(w, c, cuda)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, 1024, 1024, generator=g).to(torch.bfloat16)
    y = enc(x.to(cuda))
    ref = O.sam_image_encoder(w, Wt.SAM_PREFIX + ".image_encoder", x.float(), 2, 16, (1,))
    ref = ref.permute(0, 2, 3, 1).reshape(1, 4096, 256)
    print(f"\n[SAM blocks at ViT-H width, bf16 operands vs oracle] rel err {_rel_err(y, ref):.2e}")
    assert _rel_err(y, ref) < BOUND_SAM_BLOCKS, _rel_err(y, ref)


def test_clip_and_llama_vs_oracle(hip_lib, cuda):
    import torch

    from interactvlm_amd import llava
    from interactvlm_amd import weights as Wt
    from oracle import nn as O

    cc = Wt.ClipCfg(hidden=256, layers=4, heads=4, inter=512)
    w = _bf16_weights(Wt.clip_spec(cc))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 224, 224, generator=g).to(torch.bfloat16)
    got = llava.ClipTower(w, cc, cuda)(x.to(cuda))
    ref = O.clip_vision(w, Wt.CLIP_PREFIX, x.float(), 4, 4)
    assert got.shape == (2, 256, 256)
    print(f"\n[CLIP 4 layers, bf16 operands vs oracle] rel err {_rel_err(got, ref):.2e}")
    assert _rel_err(got, ref) < BOUND_CLIP, _rel_err(got, ref)

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1000)  # head dim 128 like LLaMA-2
    w = _bf16_weights(Wt.llama_spec(lc))
    llm = llava.Llama(w, lc, cuda, max_len=128)
    emb = (torch.randn(70, 512, generator=g) * 0.5).to(torch.bfloat16).float()  # the fp32 stream starts at bf16 embeddings
    ref = O.llama(w, "model", emb[None], 3, 4)[0]
    full = llm.forward(emb.to(cuda), 0)
    assert full.dtype == torch.float32
    print(f"[LLaMA 3 layers, bf16 operands vs oracle] rel err {_rel_err(full, ref):.2e}")
    assert _rel_err(full, ref) < BOUND_LLAMA, _rel_err(full, ref)
    # prefill 50 + 20 single-token decode steps through the KV cache == one 70-token pass
    llm2 = llava.Llama(w, lc, cuda, max_len=128)
    h = [llm2.forward(emb[:50].to(cuda), 0)]
    for t in range(50, 70):
        h.append(llm2.forward(emb[t: t + 1].to(cuda), t))
    inc = torch.cat(h, 0)
    print(f"[LLaMA prefill 50 + 20 decode steps] vs oracle {_rel_err(inc, ref):.2e}, vs the one-pass result {_rel_err(inc, full):.2e}")
    assert _rel_err(inc, ref) < BOUND_LLAMA
    assert _rel_err(inc, full) < BOUND_LLAMA  # decode rows: fp32 activations, exact products; prefill rows: bf16 MFMA operands
    # the decode rows (fp32 activations end to end) sit closer to the fp32 oracle than the bf16-operand prefill rows do
    e_dec, e_pre = _rel_err(inc[50:], ref[50:]), _rel_err(full[50:], ref[50:])
    print(f"\n[llama] decode rows vs oracle {e_dec:.2e}, the same rows through the MFMA prefill {e_pre:.2e}")
    assert e_dec < 1.5 * e_pre + 1e-3
    lg = llm.logits(full[-1:]).cpu()
    ref_lg = ref[-1:] @ w["lm_head.weight"].T
    print(f"[lm_head logits vs oracle] rel err {_rel_err(lg, ref_lg):.2e}")
    assert _rel_err(lg, ref_lg) < BOUND_LLAMA
    from interactvlm_amd import ops
    assert int(ops.argmax(llm.logits(full[-1:]))[0]) == int(lg.argmax())


@pytest.mark.parametrize("hidden,heads,inter", [(1024, 8, 1376), (512, 4, 1024)])
def test_graph_decode_with_fused_attn_oproj_matches_eager(hip_lib, cuda, hidden, heads, inter):
    """The replayed HIP graph of a decode step (position from device memory; attention + o_proj fused into one launch whose
    GEMV blocks wait on a device counter) against the eager per-op steps: same argmax ids, hidden states and KV cache."""
    import torch

    from interactvlm_amd import llava, ops
    from interactvlm_amd import weights as Wt

    lc = Wt.LlamaCfg(hidden=hidden, layers=3, heads=heads, inter=inter, vocab=1003)
    w = _bf16_weights(Wt.llama_spec(lc))
    g = torch.Generator().manual_seed(11)
    T0, n_new = 29, 14
    emb = (torch.randn(T0, hidden, generator=g) * 0.5).to(torch.bfloat16).float().to(cuda)
    toks = torch.randint(3, 1000, (n_new,), generator=g).to(torch.int32).to(cuda)

    llm_a = llava.Llama(w, lc, cuda, max_len=64)
    llm_a.forward(emb, 0)
    hid_a, arg_a = [], []
    for s in range(n_new):
        h = llm_a.forward(llm_a.embed_ids(toks[s: s + 1]), T0 + s)
        hid_a.append(h)
        arg_a.append(int(ops.argmax(llm_a.logits(h))[0]))
    llm_b = llava.Llama(w, lc, cuda, max_len=64)
    llm_b.fuse_attn_oproj = True  # (opt-in since round 2: the separate launches are as fast with gemv1_kernel)
    llm_b.forward(emb, 0)
    dg = llm_b.decode_graph()
    assert dg.get("fused") is not None
    for rep in range(2):  # a second generation re-uses the graph: counters / step / position are reset by the caller
        dg["pos"].fill_(T0)
        dg["pos64"].fill_(T0)
        for k in ("step", "counters", "status"):
            dg["fused"][k].zero_()
        hid_b, arg_b = [], []
        for s in range(n_new):
            dg["tok"].copy_(toks[s: s + 1])
            dg["graph"].replay()
            hid_b.append(dg["hidden"].clone())
            arg_b.append(int(dg["nxt"][0]))
        assert int(dg["fused"]["status"][0]) == 0
        assert int(dg["pos"][0]) == T0 + n_new and int(dg["fused"]["step"][0]) == n_new
        assert _rel_err(torch.cat(hid_b), torch.cat(hid_a).float().cpu()) < 1e-4  # same fp32 arithmetic, other launch shape
        assert _rel_err(llm_b.kcache[:, : T0 + n_new], llm_a.kcache[:, : T0 + n_new].float().cpu()) < 1e-2
        lg = torch.cat(hid_b).float().cpu() @ w["lm_head.weight"].float().T
        top2 = lg.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-2
        assert (torch.tensor(arg_b)[clear] == lg.argmax(-1)[clear]).all()


def test_decode_graph_cache_through_the_invalidation_events(hip_lib, cuda):
    """The captured decode steps are cached per (batched, B, precision, packed, fp8, fused); every event that frees or replaces a
    buffer a captured step reads drops the entries that read it.  Walked in order - a capture in the default mode, the bf16-weight
    path and back with release, decode_packed off and on, batched steps at B = 2 then B = 5 (slab growth) and B = 2 again, parity
    (lo planes), back to the default mode - after each event one replayed step equals the eager step bit for bit."""
    import torch

    from interactvlm_amd import llava, ops
    from interactvlm_amd import weights as Wt

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1003)
    w = _bf16_weights(Wt.llama_spec(lc))
    g = torch.Generator().manual_seed(23)
    T0 = 21
    emb = (torch.randn(5, T0, 512, generator=g) * 0.5).to(torch.bfloat16).float().to(cuda)
    toks = torch.randint(3, 1000, (5,), generator=g).to(torch.int32).to(cuda)
    llm = llava.Llama(w, lc, cuda, max_len=64)

    def mode(precision, packed=True, release=False):  # (what InteractVLMForCausalLM.set_precision does to the language model)
        llm.decode_packed = packed
        llm.set_precision(precision)
        llm.prepare()
        if release:
            llm.release_unused()

    def step1():  # a fresh prefill, then one step at position T0: eager, then replayed (which rewrites the same KV row)
        llm.forward(emb[0], 0)
        pos = torch.full((1,), T0, dtype=torch.int32, device=cuda)
        h = llm._decode_step(llm.embed_ids(toks[:1]), pos)
        nxt = ops.argmax(llm.logits(h))
        dg = llm.decode_graph()
        dg["pos"].fill_(T0)
        dg["tok"].copy_(toks[:1])
        dg["graph"].replay()
        assert torch.equal(dg["hidden"], h) and torch.equal(dg["nxt"], nxt) and int(dg["pos"][0]) == T0 + 1

    def step_batch(B):
        kc, vc = llm.batch_cache(B)
        lo = llm.batch_cache_lo(B) if llm.precision == "parity" else None
        for b in range(B):
            llm.forward(emb[b], 0, cache=(kc[:, b], vc[:, b]) + ((lo[0][:, b], lo[1][:, b]) if lo else ()))
        pos = torch.full((B,), T0, dtype=torch.int32, device=cuda)
        h = llm.decode_step_batch(llm.embed_ids(toks[:B]), pos, kc, vc, lo)
        nxt = ops.argmax(llm.logits(h))
        dg = llm.decode_graph_batch(B)
        dg["pos"].copy_(pos)
        dg["tok"].copy_(toks[:B])
        dg["graph"].replay()
        assert torch.equal(dg["hidden"], h) and torch.equal(dg["nxt"], nxt) and torch.equal(dg["pos"], pos + 1)
        return dg

    keys = lambda: set(llm._graphs)
    K = llava._GraphKey
    mode("f16", release=True)  # 1. the default mode (fp16 prefill, packed decode planes, bf16 matrices released)
    step1()
    assert keys() == {K(False, 1, "f16", True, False, False)}
    mode("default", packed=False)  # 2. the bf16-weight path (matrices rebuilt from the planes) ...
    step1()
    assert K(False, 1, "default", False, False, False) in keys()
    mode("f16", release=True)  # ... and back: the release drops the graph that read the rebuilt matrices
    assert keys() == {K(False, 1, "f16", True, False, False)}
    step1()
    mode("default", packed=False)  # (a new capture on the matrices rebuilt once more)
    step1()
    mode("f16", release=True)
    llm.decode_packed = False  # 3. decode_packed off (bf16 matrices rebuilt on first use) and on
    step1()
    llm.decode_packed = True
    step1()
    assert keys() == {K(False, 1, "f16", True, False, False), K(False, 1, "f16", False, False, False)}
    dg2 = step_batch(2)  # 4. batched: B = 2, then B = 5 grows the slabs and drops every batched entry, B = 2 recaptured
    step_batch(5)
    assert {k for k in keys() if k.batched} == {K(True, 5, "f16", True, False, False)}
    assert step_batch(2) is not dg2
    mode("parity")  # 5. parity: K / V as hi + lo planes (batch-1 and slab lo planes)
    step1()
    step_batch(2)
    step_batch(5)
    mode("f16", release=True)  # back: every surviving entry reads only live buffers (the release dropped the bf16-weight ones)
    assert all(k.packed for k in keys())
    dg2 = llm._graphs[K(True, 2, "f16", True, False, False)]
    assert step_batch(2) is dg2
    step1()


@pytest.mark.parametrize("precision", ["default", "f16", "parity"])
def test_packed_prefill_equals_per_sequence_prefill(hip_lib, cuda, precision):
    """forward_packed of three prompts of different lengths (one pass over the weights, one cache slab each) against
    forward(x_b, 0, cache=slab b) per prompt into a second slab: the hidden rows and every written cache row, bit for bit."""
    import torch

    from interactvlm_amd import llava
    from interactvlm_amd import weights as Wt

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1003)
    w = _bf16_weights(Wt.llama_spec(lc))
    g = torch.Generator().manual_seed(31)
    lens = (21, 40, 33)
    xs = [(torch.randn(T, 512, generator=g) * 0.5).to(torch.bfloat16).float().to(cuda) for T in lens]
    llm = llava.Llama(w, lc, cuda, max_len=64)
    llm.set_precision(precision)
    # cache planes (k, v[, k_lo, v_lo]) [layers, B, Tmax, H, hd]: fp16 K / V in "f16", hi + lo bf16 planes in "parity"
    dts = [torch.float16 if precision == "f16" else torch.bfloat16] * 2 + [torch.bfloat16] * (2 if precision == "parity" else 0)
    slab_p, slab_s = ([torch.zeros(lc.layers, len(lens), 64, 4, 128, dtype=dt, device=cuda) for dt in dts] for _ in range(2))
    hp = llm.forward_packed(xs, slab_p[0], slab_p[1], tuple(slab_p[2:]) or None)
    hs = [llm.forward(x, 0, cache=tuple(t[:, b] for t in slab_s)) for b, x in enumerate(xs)]
    for b, T in enumerate(lens):
        print(f"[{precision}] prompt {b} (T = {T}): max|dh| = {float((hp[b] - hs[b]).abs().max()):.3e}")
        assert hp[b].shape == (T, 512) and torch.equal(hp[b], hs[b])
        for tp, ts in zip(slab_p, slab_s):
            assert torch.equal(tp[:, b, :T], ts[:, b, :T])
    assert all(bool(t.any()) for t in slab_p)  # (the packed pass wrote every plane)


def _toy(golden_dir):
    import torch

    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt

    d = np.load(os.path.join(golden_dir, "model_forward_toy.npz"))
    t = json.loads(str(d["toy"]))
    cfg = Wt.IvlmCfg(
        llama=Wt.LlamaCfg(hidden=t["hidden"], layers=t["layers"], heads=t["heads"], inter=t["inter"], vocab=t["vocab"]),
        clip=Wt.ClipCfg(hidden=t["clip_hidden"], layers=t["clip_layers"], heads=t["clip_heads"], inter=t["clip_inter"]),
        sam=Wt.SamEncCfg(embed_dim=160, depth=2, num_heads=2, global_attn_indexes=(1,)))
    ids = torch.from_numpy(d["input_ids"])
    images_clip = torch.from_numpy(synth.synth_normal("mf/images_clip", (1, 3, 224, 224), 1.0, 0))
    images = torch.from_numpy(synth.synth_normal("mf/images", (1, 4, 3, 1024, 1024), 1.0, 0))
    cams = torch.from_numpy(d["cam_params"])
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    return d, cfg, ids, images_clip, images, cams, tables


def test_model_forward_vs_reference_golden(hip_lib, cuda, golden_dir):
    """The facade end to end: HIP model_forward(inference=True) vs the reference's own output."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    out = m.model_forward(images=images.to(bf).to(cuda), images_clip=images_clip.to(bf).to(cuda), input_ids=ids[None],
                          labels=None, attention_masks=torch.ones(1, len(ids)), offset=torch.tensor([0, 1]),
                          masks_list=[torch.zeros(4, 1, 1024, 1024)], label_list=[torch.zeros(1024, 1024)],
                          gt_contact_3d_list=None, cam_params=cams, resize_list=[(1024, 1024)],
                          ds_name_list=["hcontact"], mask_paths_list=[None], inference=True)
    assert set(out) == {"gt_masks", "pred_masks", "pred_human_3d_contact"}
    pm = out["pred_masks"][0]
    assert pm.shape == (4, 1024, 1024) and pm.dtype == torch.float32
    ref_pm = torch.from_numpy(d["pred_masks_sub"])
    e_mask = float((pm[..., ::16, ::16].cpu() - ref_pm).abs().max())
    contact = out["pred_human_3d_contact"].float().cpu()
    ref_c = torch.from_numpy(d["pred_contact"])
    e_c = float((contact - ref_c).abs().max())
    print(f"\n[model_forward toy] max|dmask| = {e_mask:.4f} (range {float(ref_pm.abs().max()):.2f}), "
          f"max|dp_contact| = {e_c:.2e}")
    assert contact.shape == (1, 6890)
    assert e_mask < 0.08 * float(ref_pm.abs().max())
    # same comparison against the fp32 ORACLE evaluated on the SAME bf16-rounded weights and inputs the GPU holds:
    # isolates the error of the bf16 activation path from the (unavoidable) rounding of the checkpoint itself.
    from oracle import pipeline as P
    wb = {k: (v.to(bf).float() if "gaussian" not in k else v) for k, v in w.items()}
    o = P.model_forward(wb, cfg, images[0].to(bf).float(), images_clip.to(bf).float(), ids, cams[0], tables)
    e_same = float((contact - o["pred_contact"]).abs().max())
    e_floor = float((o["pred_contact"] - ref_c).abs().max())
    print(f"[model_forward toy] vs fp32 oracle on identical bf16 weights: max|dp| = {e_same:.2e}; "
          f"bf16-checkpoint rounding floor vs fp32-weight reference: {e_floor:.2e}")
    # North-star tolerance: 1e-3 on per-vertex probabilities against the reference path on the same inputs = the fp32
    # oracle on the weights the GPU holds (bf16-representable).
    assert e_same < 1e-3, e_same
    # thresholded vertex sets equal to the oracle's off a 1e-6 band around the threshold
    oc = o["pred_contact"]
    for thr, op in ((0.5, torch.ge), (0.3, torch.gt)):
        away = (oc - thr).abs() > max(1e-6, e_same)
        assert torch.equal(op(contact, thr)[away], op(oc, thr)[away])
    # against the reference's own fp32-weight run the difference is dominated by rounding the checkpoint to bf16 (e_floor)
    assert e_c < e_floor + 1e-3, (e_c, e_floor)

    # evaluate(): KV-cached generation with the forced answer == teacher-forced pass (same [SEG] row)
    L0 = 40
    ev = m.evaluate(images_clip.to(bf).to(cuda), images.to(bf).to(cuda), ids[None, :L0], cams, [(1024, 1024)],
                    [(1024, 1024)], contact_type="hcontact", forced_new_tokens=ids[L0:].tolist())
    assert ev["output_ids"].shape == (1, len(ids)) and torch.equal(ev["output_ids"][0], ids)
    e2 = float((ev["pred_contact_3d"].float().cpu() - contact).abs().max())
    print(f"[evaluate vs model_forward] max|dp| = {e2:.2e}")
    assert e2 < 1e-3  # the answer tokens take the fp32-activation decode kernels instead of the bf16-operand MFMA prefill
    e2o = float((ev["pred_contact_3d"].float().cpu() - o["pred_contact"]).abs().max())
    print(f"[evaluate vs fp32 oracle] max|dp| = {e2o:.2e}")
    assert e2o < 1e-3
    assert float((ev["pred_masks"][0] - pm).abs().max()) < 0.08 * float(ref_pm.abs().max())
    # cached SAM embeddings give bit-identical results
    emb = m.precompute_visual_embs(images[0].to(bf).to(cuda))
    ev2 = m.evaluate(images_clip.to(bf).to(cuda), images.to(bf).to(cuda), ids[None, :L0], cams, [(1024, 1024)],
                     [(1024, 1024)], contact_type="hcontact", forced_new_tokens=ids[L0:].tolist(), image_embeddings=emb)
    assert torch.equal(ev2["pred_contact_3d"], ev["pred_contact_3d"])


def test_model_forward_oafford_vs_reference_golden(hip_lib, cuda, golden_dir, tmp_path):
    """Object-affordance branch end to end (configs[3]): an 'oafford' sample through HIP model_forward(inference=True) with
    the object predictors enabled, vs the reference's own output: sigmoid only on the non-ignored pixels of the 'HM'
    masks, point lift through the per-view p2pmap files named after the mask paths, the predictors that do not apply."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt

    d = np.load(os.path.join(golden_dir, "model_forward_oafford.npz"))
    t = json.loads(str(d["toy"]))
    cfg = Wt.IvlmCfg(
        llama=Wt.LlamaCfg(hidden=t["hidden"], layers=t["layers"], heads=t["heads"], inter=t["inter"], vocab=t["vocab"]),
        clip=Wt.ClipCfg(hidden=t["clip_hidden"], layers=t["clip_layers"], heads=t["clip_heads"], inter=t["clip_inter"]),
        sam=Wt.SamEncCfg(embed_dim=160, depth=2, num_heads=2, global_attn_indexes=(1,)), oC_loss_weight=1.0)
    ids = torch.from_numpy(d["input_ids"])
    images_clip = torch.from_numpy(synth.synth_normal("mf2/images_clip", (1, 3, 224, 224), 1.0, 0))
    images = torch.from_numpy(synth.synth_normal("mf2/images", (1, 4, 3, 1024, 1024), 1.0, 0))
    cams = torch.from_numpy(d["cam_params"])
    pid = synth.synth_point_maps(1, 4, 1024, 1024, 2048, fg=0.3, seed=int(d["point_maps_seed"]))[0]
    mask_paths = []
    for v in range(4):
        mp = str(tmp_path / f"chair_mask_{v}.png")
        np.savez(mp.replace("mask", "p2pmap")[:-4] + ".npz", mapping=pid[v])
        mask_paths.append(mp)
    gt = torch.zeros(4, 1, 1024, 1024)
    gt[:, :, : int(d["ignore_rows"])] = -1.0
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    out = m.model_forward(images=images.to(bf).to(cuda), images_clip=images_clip.to(bf).to(cuda), input_ids=ids[None],
                          labels=None, attention_masks=torch.ones(1, len(ids)), offset=torch.tensor([0, 1]),
                          masks_list=[gt], label_list=[torch.zeros(1024, 1024)], gt_contact_3d_list=None,
                          cam_params=cams, resize_list=[(1024, 1024)], ds_name_list=["oafford_piad"],
                          mask_paths_list=[mask_paths], inference=True)
    assert set(out) == {"gt_masks", "pred_masks", "pred_human_3d_contact", "pred_object_3d_contact", "pred_object_3d_afford"}
    pm = out["pred_masks"][0].float().cpu()
    ref_pm = torch.from_numpy(d["pred_masks_sub"])
    sub = pm[..., ::16, ::16]
    band = int(d["ignore_rows"]) // 16 + 1  # subsampled rows inside the IGNORE band keep raw logits
    assert float((sub[:, band:] - ref_pm[:, band:]).abs().max()) < 2e-2          # probabilities
    assert float((sub[:, :band] - ref_pm[:, :band]).abs().max()) < 0.08 * float(ref_pm[:, :band].abs().max())
    aff = out["pred_object_3d_afford"].float().cpu()
    e = float((aff - torch.from_numpy(d["pred_afford"])).abs().max())
    print(f"\n[model_forward oafford] max|dp_afford| = {e:.2e}")
    assert aff.shape == (1, 2048) and e < 2e-3
    assert tuple(out["pred_object_3d_contact"].shape) == tuple(d["pred_ocontact"].shape)
    assert float(out["pred_human_3d_contact"].abs().max()) == 0.0


def test_load_model_from_released_layout(hip_lib, cuda, tmp_path):
    """checkpoint.load_model (HF sharded safetensors + CLIP folder) builds the same model as passing the
    state dict directly: identical evaluate() outputs."""
    import torch

    from interactvlm_amd import checkpoint as C
    from interactvlm_amd import model as M
    from interactvlm_amd import synth, synthetic
    from interactvlm_amd import weights as Wt
    from _ckpt_util import _write_clip, _write_version

    cfg = synthetic.config_tiny()
    state = Wt.synth_weights(Wt.ivlm_spec(cfg))
    ver, clip = str(tmp_path / "ver"), str(tmp_path / "clip")
    _write_version(ver, cfg, state, "sharded_st")
    _write_clip(clip, state)
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m1 = C.load_model(ver, clip, cuda, lift_tables=tables)
    rounded = {k: (v if k.startswith(Wt.CLIP_PREFIX) else v.to(torch.bfloat16)) for k, v in state.items()}
    m2 = M.InteractVLMForCausalLM(cfg, rounded, cuda, lift_tables=tables)
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=6)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    o1 = m1.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced)
    o2 = m2.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced)
    assert torch.equal(o1["pred_contact_3d"], o2["pred_contact_3d"])
    assert m1.config.oC_loss_weight == 0.5  # picked up from pretrained_config.json


def test_object_render_localize_lift_flow(hip_lib, cuda, tmp_path):
    """run_demo's object path (utils/demo_utils.py:171-257 -> InteractVLM.py:620-632): normalise + rasterise a mesh under the
    four object cameras on the GPU, write the lift2d_dict.pkl the reference's predictor reads, evaluate(contact_type=
    'ocontact') -> per-vertex contacts == the C oracle's threshold lift of the same masks through the same tables."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import render, synthetic
    from interactvlm_amd import weights as Wt
    from oracle import cref
    from oracle import raster as R

    v, f = R.icosphere(3)
    v = (v * np.array([1.0, 0.6, 0.8], np.float32)).astype(np.float32)
    vid, bary, nv = render.object_lift_tables(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), "4MV-Z_HM_BM")
    assert nv == v.shape[0] and vid.shape == (4, 1024, 1024, 3)
    assert 0.05 < float((vid[..., 0] >= 0).float().mean()) < 0.8
    path = str(tmp_path / "lift2d_dict.pkl")
    render.save_lift2d_dict(path, vid, bary, nv)
    cfg = synthetic.config_tiny()
    cfg.oC_loss_weight, cfg.oC_sam_view_type = 1.0, "4MV-Z_HM_BM"
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    from interactvlm_amd import synth
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=6)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    out = m.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced,
                     contact_type="ocontact", lift2d_dict_path=path)
    pc = out["pred_contact_3d"].float().cpu().numpy()
    assert pc.shape == (1, nv)
    pm = out["pred_masks"][0].float().cpu().numpy()
    exp, _ = cref.lift_mesh_thresh(pm, vid.cpu().numpy().astype(np.int32), bary.cpu().numpy(), nv)
    # fp32 vote sums of up to a few thousand pixels per vertex, accumulated in a different order than the C oracle's
    np.testing.assert_allclose(pc, exp, atol=5e-6)
    assert np.array_equal(pc > 0.3, exp > 0.3) or np.abs(pc - exp)[(pc > 0.3) != (exp > 0.3)].max() < 5e-6

    # BASELINE.json configs[4], joint case: a human-contact prompt over the body renders AND an object prompt over the
    # object renders about ONE picture, in one call (one CLIP pass, both answers decoded together, one SAM encoder pass per
    # render set) == the two separate evaluate() calls
    m.hC_loss_weight = 1.0
    ids_o, forced_o = synthetic.prompt_ids(cfg, n_prompt=44, n_answer=8, seed=1)
    _, im_o = synthetic.images(cfg, cuda, seed=3)
    h1 = m.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced, contact_type="hcontact")
    o1 = m.evaluate(ic, im_o, ids_o, cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced_o,
                    contact_type="ocontact", lift2d_dict_path=path)
    calls = {"n": 0}
    tower = m.vision_tower.__class__.__call__

    def counting(self_, x):
        calls["n"] += 1
        return tower(self_, x)

    m.vision_tower.__class__.__call__ = counting
    try:
        both = m.evaluate_batch(ic, torch.cat([im, im_o]), [ids[0], ids_o[0]], [cams[0], cams[0]], [(1024, 1024)] * 2,
                                [(1024, 1024)] * 2, contact_type=["hcontact", "ocontact"],
                                forced_new_tokens=[forced, forced_o], lift2d_dict_path=[None, path])
    finally:
        m.vision_tower.__class__.__call__ = tower
    assert calls["n"] == 1  # one CLIP encode for both prompts
    assert both[0]["pred_contact_3d"].shape == (1, 6890) and both[1]["pred_contact_3d"].shape == (1, nv)
    for got, ref in ((both[0], h1), (both[1], o1)):
        assert torch.equal(got["output_ids"], ref["output_ids"])
        assert float((got["pred_contact_3d"] - ref["pred_contact_3d"]).abs().max()) < 1e-3
        assert float((got["pred_masks"][0] - ref["pred_masks"][0]).abs().max()) < 0.05


def test_decode_attn_batch_equals_per_sequence(hip_lib, cuda):
    """ivlm_llama_decode_attn_batch (grid heads x sequences, one cache slab and one position per sequence) is bit-identical
    to B separate single-sequence launches, including the appended cache rows."""
    import torch

    from interactvlm_amd import ops

    B, H, D, Tmax = 5, 8, 128, 96
    g = torch.Generator().manual_seed(3)
    qkv = (torch.randn(B, 3 * H * D, generator=g)).to(torch.bfloat16).to(cuda)
    kc = (torch.randn(B, Tmax, H, D, generator=g)).to(torch.bfloat16).to(cuda)
    vc = (torch.randn(B, Tmax, H, D, generator=g)).to(torch.bfloat16).to(cuda)
    pos = torch.tensor([0, 17, 63, 64, 95], dtype=torch.int32, device=cuda)
    tab = ops.rope_table(Tmax, D, 10000.0, cuda)
    kc1, vc1 = kc.clone(), vc.clone()
    exp = torch.cat([ops.llama_decode_attn(qkv[b: b + 1].contiguous(), kc1[b], vc1[b], H, D, int(pos[b]), 10000.0,
                                           D ** -0.5, table=tab) for b in range(B)])
    got = ops.llama_decode_attn_batch(qkv, kc, vc, H, D, pos, 10000.0, D ** -0.5, table=tab)
    assert torch.equal(got, exp) and torch.equal(kc, kc1) and torch.equal(vc, vc1)
    with pytest.raises(AssertionError):
        ops.llama_decode_attn_batch(qkv, kc, vc, H, D, pos[:3], 10000.0, D ** -0.5, table=tab)
    # fp32 I/O (the decode path proper): against torch fp64 on the bf16 cache + the exact new row; a sequence whose position
    # has reached the end of its slab is skipped (nothing appended, its neighbour's slab untouched)
    q32 = torch.randn(B, 3 * H * D, generator=g).to(cuda)
    pos2 = torch.tensor([0, 17, 63, 64, Tmax], dtype=torch.int32, device=cuda)
    kc2, vc2 = kc.clone(), vc.clone()
    got32 = ops.llama_decode_attn_batch(q32, kc2, vc2, H, D, pos2, 10000.0, D ** -0.5, table=tab)
    assert got32.dtype == torch.float32 and torch.equal(kc2[4], kc[4]) and torch.equal(vc2[4], vc[4])
    assert float(got32[4].abs().max()) == 0.0
    cos, sin = tab[0].double().cpu(), tab[1].double().cpu()
    for b in range(4):
        p = int(pos2[b])
        x = q32[b].double().cpu().view(3, H, D)
        c, s_ = torch.cat([cos[p], cos[p]]), torch.cat([sin[p], sin[p]])
        rot = lambda t: torch.cat([-t[..., D // 2:], t[..., : D // 2]], -1)
        qr, kr = x[0] * c + rot(x[0]) * s_, x[1] * c + rot(x[1]) * s_
        K_ = torch.cat([kc[b, :p].double().cpu(), kr[None]], 0)  # [p+1, H, D]: bf16 history + exact new row
        V_ = torch.cat([vc[b, :p].double().cpu(), x[2][None]], 0)
        a = torch.softmax(torch.einsum("hd,thd->ht", qr, K_) * D ** -0.5, -1)
        ref = torch.einsum("ht,thd->hd", a, V_).reshape(-1)
        assert float((got32[b].double().cpu() - ref).abs().max()) < 2e-5, b
        assert torch.equal(kc2[b, p], kr.to(torch.bfloat16).to(cuda)) or \
            float((kc2[b, p].double().cpu() - kr).abs().max()) < 2.0 ** -7 * float(kr.abs().max())


@pytest.mark.parametrize("graph", [True, False])
def test_evaluate_batch_equals_per_image_evaluate(hip_lib, cuda, golden_dir, graph):
    """evaluate_batch (BASELINE.json configs[2]: several images per GPU - prompts of different lengths, one decode step
    streaming the weights once for all sequences) returns, image by image, what evaluate() returns for that image alone:
    same ids bit for bit, contacts within the GEMV-row tolerance (M = B vs M = 1 kernels share the summation order)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    m.graph_decode = graph
    bf = torch.bfloat16
    B = 3
    ic = torch.from_numpy(synth.synth_normal("eb/images_clip", (B, 3, 224, 224), 1.0, 0)).to(bf).to(cuda)
    im = torch.from_numpy(synth.synth_normal("eb/images", (B, 4, 3, 1024, 1024), 1.0, 0)).to(bf).to(cuda)
    L0 = [40, 36, 40]  # prompt lengths differ: the sequences sit at different positions in every step
    prompts, forced = [], []
    for b in range(B):
        p = ids[: L0[b]].clone()
        if b == 1:
            p = torch.cat([ids[:30], ids[34:40]])
        prompts.append(p)
        forced.append(ids[40:].tolist() if b != 2 else ids[40: len(ids) - 2].tolist() + [int(ids[-1])])
    cam_b = [cams[0]] * B
    sizes = [(1024, 1024)] * B
    single = [m.evaluate(ic[b: b + 1], im[b: b + 1], prompts[b][None], cams, [(1024, 1024)], [(1024, 1024)],
                         forced_new_tokens=forced[b]) for b in range(B)]
    outs = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced)
    assert len(outs) == B
    for b in range(B):
        assert torch.equal(outs[b]["output_ids"], single[b]["output_ids"])
        e = float((outs[b]["pred_contact_3d"] - single[b]["pred_contact_3d"]).abs().max())
        em = float((outs[b]["pred_masks"][0] - single[b]["pred_masks"][0]).abs().max())
        print(f"\n[evaluate_batch graph={graph}] image {b}: max|dp| = {e:.2e}, max|dmask| = {em:.3e}")
        assert outs[b]["pred_contact_3d"].shape == (1, 6890)
        assert e < 1e-3
    # free-running greedy search: every sequence stops at its own EOS / length, ids equal the per-image runs
    free1 = [m.evaluate(ic[b: b + 1], im[b: b + 1], prompts[b][None], cams, [(1024, 1024)], [(1024, 1024)],
                        max_new_tokens=6 + b, eos_token_id=-1)["output_ids"] for b in range(B)]
    free = m.generate_batch(ic, prompts, max_new_tokens=8, eos_token_id=-1)
    for b in range(B):
        n = min(free1[b].shape[1], free[b][0].shape[1])
        assert torch.equal(free1[b][0, :n], free[b][0][0, :n])
    # a second call re-uses the captured graph and the cache slabs
    outs2 = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced)
    for b in range(B):
        assert torch.equal(outs2[b]["pred_contact_3d"], outs[b]["pred_contact_3d"])
    # pre-computed SAM embeddings (8f-1), one tensor per image: same results without running the encoder
    embs = [m.precompute_visual_embs(im[b]) for b in range(B)]
    outs3 = m.evaluate_batch(ic, None, prompts, cam_b, sizes, sizes, forced_new_tokens=forced, image_embeddings=embs)
    for b in range(B):
        assert torch.equal(outs3[b]["pred_contact_3d"], outs[b]["pred_contact_3d"])


@pytest.mark.parametrize("B", [16, 17])
def test_evaluate_batch_of_16_and_chunking(hip_lib, cuda, golden_dir, B):
    """The decode kernels' row limit: 16 sequences in one batched step (the dp64 job's per-call batch), 17 = one call of 16 + one
    of 1 - every image equal to evaluate() of that image alone."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    ic = torch.from_numpy(synth.synth_normal("eb16/images_clip", (B, 3, 224, 224), 1.0, 0)).to(bf).to(cuda)
    im = torch.from_numpy(synth.synth_normal("eb16/images", (B, 4, 3, 1024, 1024), 1.0, 0)).to(bf).to(cuda)
    prompts = [ids[:40] if b % 3 else torch.cat([ids[:30], ids[34:40]]) for b in range(B)]
    forced = [ids[40:].tolist()] * B
    sizes = [(1024, 1024)] * B
    outs = m.evaluate_batch(ic, im, prompts, [cams[0]] * B, sizes, sizes, forced_new_tokens=forced)
    assert len(outs) == B
    for b in (0, 7, 9, 15, B - 1):
        one = m.evaluate(ic[b: b + 1], im[b: b + 1], prompts[b][None], cams, [(1024, 1024)], [(1024, 1024)], forced_new_tokens=forced[b])
        assert torch.equal(outs[b]["output_ids"], one["output_ids"])
        e = float((outs[b]["pred_contact_3d"] - one["pred_contact_3d"]).abs().max())
        assert e < 1e-3, (b, e)
    if B == 17:
        # deferred chunks: chunk c + 1 is begun (its SAM encoder, CLIP, prefill and decode loop enqueued) before
        # chunk c's tail - the mask decoders and the lift - is enqueued; same results, bit for bit, as the calls one after the other
        from interactvlm_amd import dist as D

        sl = lambda lo, hi: (ic[lo:hi], im[lo:hi], prompts[lo:hi], [cams[0]] * (hi - lo), sizes[lo:hi], sizes[lo:hi])
        fins = [m.evaluate_batch(*sl(0, 6), forced_new_tokens=forced[0:6], deferred=True)]
        fins.append(m.evaluate_batch(*sl(6, 11), forced_new_tokens=forced[6:11], deferred=True))  # begun before chunk 0 is finished
        piped = fins[0]() + fins[1]()
        plain = m.evaluate_batch(*sl(0, 6), forced_new_tokens=forced[0:6]) + m.evaluate_batch(*sl(6, 11), forced_new_tokens=forced[6:11])
        for a_, b_ in zip(piped, plain):
            assert torch.equal(a_["output_ids"], b_["output_ids"]) and torch.equal(a_["pred_contact_3d"], b_["pred_contact_3d"])
            assert torch.equal(a_["pred_masks"][0], b_["pred_masks"][0])
        # ... and through dist.evaluate_sharded, whose chunk callback may return the deferred function
        chunk = lambda idx: (lambda f: (lambda: torch.cat([o["pred_contact_3d"] for o in f()])))(
            m.evaluate_batch(ic[idx], im[idx], [prompts[i] for i in idx], [cams[0]] * len(idx), [sizes[i] for i in idx],
                             [sizes[i] for i in idx], forced_new_tokens=[forced[i] for i in idx], deferred=True))
        got = D.evaluate_sharded(11, 4, chunk, rank=0, world=1)
        assert torch.equal(got, torch.cat([o["pred_contact_3d"] for o in plain]))


def test_full_depth_towers_vs_oracle(hip_lib, cuda):
    """Parity evidence at the REAL depths (evidence stopped at depth 2-4): the SAM ViT-H encoder with all 32
    blocks at its real width on one view, and a 32-layer LLaMA (narrower: the fp32 CPU oracle of the 7B width would need
    27 GB of weights), HIP vs the fp32 oracle on identical bf16-representable weights.  The measured error levels are
    printed; the bounds are what bf16 MFMA operands over an fp32 residual stream give at this depth (per block ~0.5 % of
    relative rms noise from the operand roundings - normed rows, q / k / v, softmax weights, attention output, MLP hidden -
    adding in quadrature over 32 blocks; the reference's own bf16 model rounds the stream as well and sits further out)."""
    import time

    import torch

    from interactvlm_amd import llava, sam
    from interactvlm_amd import weights as Wt
    from oracle import nn as O

    torch.set_grad_enabled(False)
    c = Wt.SamEncCfg()  # ViT-H: 32 blocks, 1280 wide, 16 heads, global blocks 7/15/23/31
    w = _bf16_weights(Wt.sam_encoder_spec(c))
    enc = sam.SamImageEncoder(w, c, cuda)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, 1024, 1024, generator=g).to(torch.bfloat16)
    y = enc(x.to(cuda)).float().cpu()
    t0 = time.time()
    ref = O.sam_image_encoder(w, Wt.SAM_PREFIX + ".image_encoder", x.float(), c.depth, c.num_heads, c.global_attn_indexes)
    ref = ref.permute(0, 2, 3, 1).reshape(1, 4096, 256)
    rel_rms = float((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"\n[SAM ViT-H, 32 blocks, 1 view] rel rms err {rel_rms:.4f}, max abs {float((y - ref).abs().max()):.3f} of "
          f"{float(ref.abs().max()):.2f} (oracle {time.time() - t0:.0f} s)")
    assert rel_rms < 8e-2
    del enc, w

    lc = Wt.LlamaCfg(hidden=1024, layers=32, heads=8, inter=2752, vocab=1000)
    w = _bf16_weights(Wt.llama_spec(lc))
    llm = llava.Llama(w, lc, cuda, max_len=256)
    emb = (torch.randn(160, 1024, generator=g) * 0.5).to(torch.bfloat16).float()
    ref = O.llama(w, "model", emb[None], lc.layers, lc.heads)[0]
    h = [llm.forward(emb[:140].to(cuda), 0)]
    for t in range(140, 160):
        h.append(llm.forward(emb[t: t + 1].to(cuda), t))
    got = torch.cat(h, 0).cpu()
    e_pre = float((got[:140] - ref[:140]).pow(2).mean().sqrt() / ref[:140].pow(2).mean().sqrt())
    e_dec = float((got[140:] - ref[140:]).pow(2).mean().sqrt() / ref[140:].pow(2).mean().sqrt())
    print(f"[LLaMA 32 layers] rel rms err: prefill rows (bf16 MFMA operands) {e_pre:.4f}, decode rows (fp32 activations) {e_dec:.4f}")
    assert e_pre < 2e-2 and e_dec < 2e-2


@pytest.mark.parametrize("kind", ["simple", "view_index", "vi_v1"])
def test_cam_encoders_and_attention_splitter_vs_reference_golden(hip_lib, cuda, golden_dir, kind):
    """process_embeddings on the HIP path for every conditioning branch of the reference (components.py:491-571 CamPoseEncoder
    / ViewIndexCamPoseEncoder / VIv1CamPoseEncoder; AttentionSplitter :155-193 for token_type 'Gen-Hu-Obj' with the human and
    the object [SEG] tokens; InteractVLM.py:268-294) against the goldens produced by the reference's own classes.  The
    activations are fp32 on this path, the weights the golden's fp32 values rounded to bf16."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt

    d = np.load(os.path.join(golden_dir, "cam_encoders.npz"))
    cams = torch.from_numpy(d["cam_params"])
    emb = torch.from_numpy(synth.synth_normal("cam/seg_emb", (1, 1, 256), 1.0, 0)).repeat(1, 4, 1)
    w = Wt.synth_weights({**Wt.cam_encoder_spec(kind), **Wt.attention_splitter_spec()})
    for tt in ("Gen", "Gen-Hu-Obj"):
        m = M.InteractVLMForCausalLM.__new__(M.InteractVLMForCausalLM)  # only the conditioning sub-modules
        m.device = cuda
        m.multiview_cam_cond, m.cam_encoder_type, m.base_token_type = True, kind, tt
        m.hseg_token_idx, m.oseg_token_idx = 32003, 32004
        m.cam_pose_encoder = M._CamPoseEncoder(w, kind, 4, cuda)
        m.attention_splitter = {n: M._Lin(w, "attention_splitter." + n, cuda) for n in
                                ("input_proj", "query_human", "query_object", "key", "value", "output_proj")}
        for token in ((32000,) if tt == "Gen" else (32000, 32003, 32004)):
            got = m.process_embeddings(emb.to(cuda), cams, token).float().cpu()
            ref = torch.from_numpy(d[f"{kind}/{tt}/{token}"])
            err = float((got - ref).abs().max())
            print(f"\n[process_embeddings {kind}/{tt}/{token}] max abs err {err:.2e} (range {float(ref.abs().max()):.2f})")
            assert got.shape == ref.shape and err < 1.5e-2 * float(ref.abs().max())  # bf16-rounded weights vs fp32 weights
            # against the fp32 oracle on the SAME bf16-rounded weights: fp32 activations, exact products
            from oracle import nn as O
            wb = {k: v.to(torch.bfloat16).float() for k, v in w.items()}
            cfg = dict(multiview_cam_cond=True, cam_encoder_type=kind, multiview_channels=4, base_token_type=tt,
                       hseg_token_idx=32003, oseg_token_idx=32004)
            o = O.process_embeddings(wb, emb.clone(), cams, token, cfg)
            assert float((got - o).abs().max()) < 2e-5 * max(1.0, float(o.abs().max())), (kind, tt, token)


def test_model_forward_gen_hu_obj_vs_reference_golden(hip_lib, cuda, golden_dir):
    """The facade with token_type 'Gen-Hu-Obj' ([HSEG] answer token -> AttentionSplitter human branch, 'view_index' camera
    encoder) against the reference's own model_forward(inference=True) output and the fp32 oracle on identical weights."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt
    from oracle import pipeline as P

    d = np.load(os.path.join(golden_dir, "model_forward_huobj.npz"))
    t = json.loads(str(d["toy"]))
    cfg = Wt.IvlmCfg(
        llama=Wt.LlamaCfg(hidden=t["hidden"], layers=t["layers"], heads=t["heads"], inter=t["inter"], vocab=t["vocab"]),
        clip=Wt.ClipCfg(hidden=t["clip_hidden"], layers=t["clip_layers"], heads=t["clip_heads"], inter=t["clip_inter"]),
        sam=Wt.SamEncCfg(embed_dim=160, depth=2, num_heads=2, global_attn_indexes=(1,)), token_type="Gen-Hu-Obj",
        cam_encoder_type="view_index", hseg_token_idx=31999, oseg_token_idx=31998)
    ids = torch.from_numpy(d["input_ids"])
    images_clip = torch.from_numpy(synth.synth_normal("mf/images_clip", (1, 3, 224, 224), 1.0, 0))
    images = torch.from_numpy(synth.synth_normal("mf/images", (1, 4, 3, 1024, 1024), 1.0, 0))
    cams = torch.from_numpy(d["cam_params"])
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    assert m.attention_splitter is not None
    bf = torch.bfloat16
    out = m.model_forward(images=images.to(bf).to(cuda), images_clip=images_clip.to(bf).to(cuda), input_ids=ids[None],
                          offset=torch.tensor([0, 1]), masks_list=[torch.zeros(4, 1, 1024, 1024)],
                          label_list=[torch.zeros(1024, 1024)], cam_params=cams, resize_list=[(1024, 1024)],
                          ds_name_list=["hcontact"], mask_paths_list=[None], inference=True)
    contact = out["pred_human_3d_contact"].float().cpu()
    wb = {k: (v.to(bf).float() if "gaussian" not in k else v) for k, v in w.items()}
    o = P.model_forward(wb, cfg, images[0].to(bf).float(), images_clip.to(bf).float(), ids, cams[0], tables)
    e_same = float((contact - o["pred_contact"]).abs().max())
    e_ref = float((contact - torch.from_numpy(d["pred_contact"])).abs().max())
    e_floor = float((o["pred_contact"] - torch.from_numpy(d["pred_contact"])).abs().max())
    print(f"\n[model_forward Gen-Hu-Obj] vs fp32 oracle on identical weights {e_same:.2e}; vs reference golden {e_ref:.2e} "
          f"(bf16-checkpoint floor {e_floor:.2e})")
    assert e_same < 1e-3 and e_ref < e_floor + 1e-3
    # evaluate(): the [HSEG] token arrives through generation, same branch
    L0 = 40
    ev = m.evaluate(images_clip.to(bf).to(cuda), images.to(bf).to(cuda), ids[None, :L0], cams, [(1024, 1024)], [(1024, 1024)],
                    contact_type="hcontact", forced_new_tokens=ids[L0:].tolist())
    assert float((ev["pred_contact_3d"].float().cpu() - o["pred_contact"]).abs().max()) < 1e-3


def test_difde_decoders_selected_by_dataset_name(hip_lib, cuda):
    """'-DifDe' token types: the human / object mask decoders are separately trained modules picked per sample by dataset name
    (InteractVLM.py:46-52, 114-121).  A '-DifDe' model with three different decoders must produce, for an hcontact
    sample, exactly what a plain model holding the human decoder's weights as mask_decoder.* produces - and likewise for the
    object decoder on 'ocontact' / 'oafford' names and the shared one on anything else."""
    import dataclasses

    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth, synthetic
    from interactvlm_amd import weights as Wt

    cfg = dataclasses.replace(synthetic.config_tiny(), token_type="Gen-DifDe", difde_load="separate")
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    assert any(".human_mask_decoder." in k for k in w) and any(".object_mask_decoder." in k for k in w)
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    vm = m.model.visual_model
    assert m._mask_decoder_for("hcontact_damon") is vm.human_mask_decoder
    assert m._mask_decoder_for("oafford_piad") is vm.object_mask_decoder and m._mask_decoder_for("ocontact_x") is vm.object_mask_decoder
    assert m._mask_decoder_for("other") is vm.mask_decoder and m._mask_decoder_for(None) is vm.mask_decoder
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    out = m.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], contact_type="hcontact", forced_new_tokens=forced)
    emb = m.precompute_visual_embs(im[0])
    text = torch.randn(1, 4, 256, device=cuda)
    for name in ("human_mask_decoder", "object_mask_decoder"):
        w2 = {k: v for k, v in w.items() if ".human_mask_decoder." not in k and ".object_mask_decoder." not in k}
        w2.update({k.replace("." + name + ".", ".mask_decoder."): v for k, v in w.items() if "." + name + "." in k})
        m2 = M.InteractVLMForCausalLM(dataclasses.replace(cfg, token_type="Gen"), w2, cuda, lift_tables=tables)
        low_a, iou_a = getattr(vm, name)(emb, text)
        low_b, iou_b = m2.model.visual_model.mask_decoder(emb, text)
        assert torch.equal(low_a, low_b) and torch.equal(iou_a, iou_b)
        low_c, _ = vm.mask_decoder(emb, text)
        assert not torch.equal(low_a, low_c)  # the three decoders really are different modules
        if name == "human_mask_decoder":
            out2 = m2.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], contact_type="hcontact", forced_new_tokens=forced)
            assert torch.equal(out["pred_masks"][0], out2["pred_masks"][0])
            assert torch.equal(out["pred_contact_3d"], out2["pred_contact_3d"])
        del m2


def test_difde_reference_load_semantics_switch(hip_lib, cuda):
    """a '-DifDe' checkpoint whose three decoder copies DIFFER.  Default (difde_load = "reference"): the reference's
    from_pretrained-into-aliased-modules-then-deepcopy construction (InteractVLM.py:30-32, evaluate.py:557-563) - all three decoders
    hold object_mask_decoder.*, i.e. what the reference evaluates on the same checkpoint.  difde_load = "separate" (opt-in): each
    decoder its own tensors.  The loader warns that the copies differ and says which semantics is applied."""
    import dataclasses
    import warnings

    import torch

    from interactvlm_amd import checkpoint
    from interactvlm_amd import model as M
    from interactvlm_amd import synth, synthetic
    from interactvlm_amd import weights as Wt

    cfg = dataclasses.replace(synthetic.config_tiny(), token_type="Gen-DifDe")
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))  # (the three decoders are distinct tensors: keyed random draws)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert checkpoint.warn_if_difde_copies_differ(w, cfg)
    assert cfg.difde_load == "reference"  # (the drop-in default)
    assert any("difde_load='reference'" in str(r.message) for r in rec)
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    ev = lambda m_: m_.evaluate(ic, im, ids, cams, [(1024, 1024)], [(1024, 1024)], contact_type="hcontact", forced_new_tokens=forced)
    sep = ev(M.InteractVLMForCausalLM(dataclasses.replace(cfg, difde_load="separate"), w, cuda, lift_tables=tables))
    ref_sem = ev(M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables))
    # "reference": hcontact goes through a decoder holding object_mask_decoder.* == a plain model whose mask_decoder.* are those tensors
    pre = Wt.SAM_PREFIX
    w_obj = {k: v for k, v in w.items() if "human_mask_decoder" not in k and "object_mask_decoder" not in k}
    for k, v in w.items():
        if k.startswith(pre + ".object_mask_decoder."):
            w_obj[pre + ".mask_decoder." + k[len(pre + ".object_mask_decoder."):]] = v
    plain = ev(M.InteractVLMForCausalLM(dataclasses.replace(cfg, token_type="Gen"), w_obj, cuda, lift_tables=tables))
    assert torch.equal(ref_sem["pred_contact_3d"], plain["pred_contact_3d"])
    assert not torch.equal(sep["pred_contact_3d"], ref_sem["pred_contact_3d"])  # (the copies differ: so do the two semantics)


def test_forward_with_past_key_values_is_the_causal_lm_forward(hip_lib, cuda):
    """forward(past_key_values=...) (InteractVLM.py:263-266 -> llava_llama.py:55-135): a greedy loop driven through it - full
    sequence first, then one id at a time against the cache handle - yields the ids and hidden states of generate(); with
    past_key_values=None every call re-runs the whole sequence (the reference's use_cache=False behaviour)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth, synthetic
    from interactvlm_amd import weights as Wt

    cfg = synthetic.config_tiny()
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=synth.synth_mesh_tables(4, 64, 64, 6890, fg=0.4, seed=0))
    m.graph_decode = False
    ids, _ = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    ic, _ = synthetic.images(cfg, cuda)
    out_ids, hidden = m.generate(ic, ids, max_new_tokens=6, eos_token_id=-1)
    new = out_ids[0, ids.shape[1]:].tolist()
    o = m.forward(input_ids=ids, images=ic, past_key_values=None, use_cache=True)
    assert o.logits.shape == (1, ids.shape[1] + cfg.img_emb_len, cfg.llama.vocab) and o.past_key_values.length == hidden.shape[0] - 5
    got = [int(o.logits[0, -1].argmax())]
    cur = ids
    for _ in range(5):
        cur = torch.cat([cur, torch.tensor([[got[-1]]])], 1)
        o = m.forward(input_ids=cur, past_key_values=o.past_key_values, use_cache=True)
        assert o.logits.shape[1] == 1
        got.append(int(o.logits[0, -1].argmax()))
    assert got == new
    # stateless form: the whole sequence again, same last-row logits as the cached step
    o2 = m.forward(input_ids=cur, images=ic, past_key_values=None)
    assert o2.past_key_values is None and int(o2.logits[0, -1].argmax()) == got[-1]
    assert torch.allclose(o2.hidden_states[0, -1], o.hidden_states[0, -1], atol=2e-2, rtol=2e-2)


def test_free_running_generation_vs_oracle_greedy(hip_lib, cuda, golden_dir):
    """generate() / generate_batch() (KV-cached greedy search) against the ORACLE's restatement of the reference's
    loop - uncached full re-forwards + argmax, stop on EOS / max_new_tokens (oracle.pipeline.greedy = InteractVLM.py:524-531 with
    use_cache False) - token by token.  A step is compared wherever the oracle's top-2 logit margin exceeds the tolerance of the
    HIP logits (measured here against the oracle's logits of the same prefix); once a below-tolerance step differs the prefixes
    diverge legitimately and the comparison stops.  Also: one B = 16 evaluate_batch contact vector directly against the oracle."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synthetic
    from interactvlm_amd import weights as Wt
    from oracle import pipeline as P

    torch.set_grad_enabled(False)
    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = {k: v.to(torch.bfloat16).float() for k, v in Wt.synth_weights(Wt.ivlm_spec(cfg)).items()}
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    n_new, compared = 10, 0
    prompts = [ids[:40], torch.cat([ids[:30], ids[34:40]]), ids[:38]]
    ics = [images_clip.to(bf), (images_clip * 0.5 + 0.1).to(bf), (-images_clip).to(bf)]
    refs = [P.greedy(w, cfg, ics[b].float(), prompts[b], max_new_tokens=n_new, eos_token_id=2) for b in range(3)]
    for graph in (True, False):
        m.graph_decode = graph
        outs = [m.generate(ics[b].to(cuda), prompts[b][None], max_new_tokens=n_new, eos_token_id=2) for b in range(3)]
        outs_b = m.generate_batch(torch.cat(ics).to(cuda), prompts, max_new_tokens=n_new, eos_token_id=2)
        for b in range(3):
            ref_ids, margins, ref_logits = refs[b]
            L = prompts[b].shape[0]
            for name, (got_ids, hidden) in (("generate", outs[b]), ("generate_batch", outs_b[b])):
                got = got_ids[0, L:].tolist()
                want = ref_ids[L:].tolist()
                # tolerance of the HIP logits: lm_head on the HIP hidden state of the step's last prefix row vs the oracle's logits
                for t in range(min(len(got), len(want))):
                    row = hidden[L + cfg.img_emb_len - 1 + t]  # (the prompt occupies L + img_emb_len positions: one id -> 256 rows)
                    lg = row.float().cpu() @ w["lm_head.weight"].t()
                    tol = 2.0 * float((lg - ref_logits[t]).abs().max())
                    if float(margins[t]) <= tol:
                        if got[t] != want[t]:
                            break  # an undecidable step went the other way: the prefixes differ from here on
                        continue
                    assert got[t] == want[t], (name, graph, b, t, got, want, float(margins[t]), tol)
                    compared += 1
                else:
                    assert len(got) == len(want), (name, got, want)  # same stop (EOS / max_new_tokens)
    print(f"\n[free-running greedy vs oracle] {compared} decidable steps compared, all equal")
    assert compared >= 40
    # one B = 16 batched call: a contact vector straight against the oracle (not only against evaluate() of the same image)
    from interactvlm_amd import synth
    B = 16
    ic = torch.from_numpy(synth.synth_normal("eb16/images_clip", (B, 3, 224, 224), 1.0, 0)).to(bf)
    im = torch.from_numpy(synth.synth_normal("eb16/images", (B, 4, 3, 1024, 1024), 1.0, 0)).to(bf)
    forced = ids[40:].tolist()
    outs = m.evaluate_batch(ic.to(cuda), im.to(cuda), [ids[:40]] * B, [cams[0]] * B, [(1024, 1024)] * B, [(1024, 1024)] * B,
                            forced_new_tokens=[forced] * B)
    for b in (5, 15):
        ref = P.model_forward(w, cfg, im[b].float(), ic[b: b + 1].float(), ids, cams[0], tables)["pred_contact"]
        e = float((outs[b]["pred_contact_3d"].float().cpu() - ref).abs().max())
        print(f"[evaluate_batch(16) image {b} vs oracle] max |dp| = {e:.2e}")
        assert e < 1e-3


def test_free_running_generation_stops_on_eos_one_step_late(hip_lib, cuda, golden_dir):
    """the graph-replay greedy loop no longer reads the new id back before it enqueues the next step - ids stay on
    the device, a pinned host copy is polled ONE step late, so when id k is EOS one speculative step has been enqueued and must be
    dropped.  Random weights never emit a given EOS, so the EOS id is chosen from what the model generates: for every cut point
    k the graph loop must return exactly the eager loop's result (ids up to and including the first EOS, hidden rows up to the row
    that predicted it), for generate() and for generate_batch() with sequences that stop at different steps - and the next call
    must not see anything of the dropped step (same result again)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt

    torch.set_grad_enabled(False)
    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    prompts = [ids[:40], torch.cat([ids[:30], ids[34:40]]), ids[:38]]
    ics = [images_clip.to(bf).to(cuda), (images_clip * 0.5 + 0.1).to(bf).to(cuda), (-images_clip).to(bf).to(cuda)]
    n_new = 9
    m.graph_decode = True
    free = [m.generate(ics[b], prompts[b][None], max_new_tokens=n_new, eos_token_id=-1) for b in range(3)]
    for b in range(3):
        L = prompts[b].shape[0]
        new = free[b][0][0, L:].tolist()
        assert len(new) == n_new and free[b][1].shape[0] == L + cfg.img_emb_len + n_new - 1
        for k in (0, 1, 4, n_new - 2, n_new - 1):
            eos = new[k]
            first = new.index(eos)  # (an id may repeat: the loop stops at its FIRST occurrence)
            for graph in (True, False, True):
                m.graph_decode = graph
                got_ids, hidden = m.generate(ics[b], prompts[b][None], max_new_tokens=n_new, eos_token_id=eos)
                assert got_ids[0, L:].tolist() == new[: first + 1], (b, k, graph)
                assert hidden.shape[0] == L + cfg.img_emb_len + first
                assert torch.equal(hidden, free[b][1][: hidden.shape[0]]), (b, k, graph)
    # batched: the three sequences stop at different steps (an EOS id that sequence 1 emits at step 2; the others may never emit it)
    m.graph_decode = False
    free_b = m.generate_batch(torch.cat(ics), prompts, max_new_tokens=n_new, eos_token_id=-1)
    L1 = prompts[1].shape[0]
    eos = free_b[1][0][0, L1 + 2].item()
    want = []
    for b in range(3):
        new = free_b[b][0][0, prompts[b].shape[0]:].tolist()
        assert len(new) == n_new
        want.append(new[: new.index(eos) + 1] if eos in new else new)
    assert len(want[1]) <= 3
    for graph in (True, False, True):
        m.graph_decode = graph
        outs = m.generate_batch(torch.cat(ics), prompts, max_new_tokens=n_new, eos_token_id=eos)
        for b in range(3):
            L = prompts[b].shape[0]
            assert outs[b][0][0, L:].tolist() == want[b], (b, graph)
            assert outs[b][1].shape[0] == L + cfg.img_emb_len + len(want[b]) - 1
            assert torch.equal(outs[b][1], free_b[b][1][: outs[b][1].shape[0]]), (b, graph)


@pytest.mark.parametrize("cache_dtype", ["bf16", "f16"])
def test_decode_attn_splitkv_equals_one_block_kernel(hip_lib, cuda, cache_dtype):
    """The split-KV decode attention (H x S blocks, the last block of a head merges the range partials) against the one-block-per-head
    kernel: same output up to the fp32 summation order, the SAME appended cache rows, at positions that leave ranges empty (0, 5),
    fill exactly one tile, straddle tiles, need several tiles per range (3000), and past the slab (zeros, nothing appended); for every
    split count; repeated launches on one scratch (the counters are left at zero); device and host positions."""
    import torch

    from interactvlm_amd import ops

    H, D, Tmax = 8, 128, 3072
    dt = torch.bfloat16 if cache_dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(11)
    kc0 = torch.randn(Tmax, H, D, generator=g).to(dt).to(cuda)
    vc0 = torch.randn(Tmax, H, D, generator=g).to(dt).to(cuda)
    tab = ops.rope_table(Tmax, D, 10000.0, cuda)
    scratch = ops.decode_attn_scratch(H, D, cuda)
    try:
        for splits in (8, 1, 3, 16):
            assert hip_lib.ivlm_llama_decode_attn_splits(splits) == 0
            for pos in (0, 5, 95, 96, 650, 767, 768, 3000, Tmax - 1):
                qkv = torch.randn(1, 3 * H * D, generator=g).to(cuda)
                k1, v1, k2, v2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
                ref = ops.llama_decode_attn(qkv, k1, v1, H, D, pos, 10000.0, D ** -0.5, table=tab)
                p_arg = torch.tensor([pos], dtype=torch.int32, device=cuda) if pos % 2 else pos
                got = ops.llama_decode_attn(qkv, k2, v2, H, D, p_arg, 10000.0, D ** -0.5, table=tab, scratch=scratch)
                assert torch.equal(k1, k2) and torch.equal(v1, v2), (splits, pos)
                err = float((got - ref).abs().max())
                assert err < 2e-6 * max(1.0, float(ref.abs().max())), (splits, pos, err)
            assert int(scratch[:H * 4].view(torch.int32).abs().max()) == 0
        assert hip_lib.ivlm_llama_decode_attn_splits(17) != 0 and hip_lib.ivlm_llama_decode_attn_splits(0) != 0
        # past the slab: zeros, nothing appended
        small_k, small_v = kc0[:64].clone(), vc0[:64].clone()
        out = ops.llama_decode_attn(torch.randn(1, 3 * H * D, generator=g).to(cuda), small_k, small_v, H, D,
                                    torch.tensor([64], dtype=torch.int32, device=cuda), 10000.0, D ** -0.5, table=tab, scratch=scratch)
        assert float(out.abs().max()) == 0.0 and torch.equal(small_k, kc0[:64]) and torch.equal(small_v, vc0[:64])
        # small heads (D = 16: one 16-byte chunk per row), H not a power of two
        H2, D2 = 5, 16
        kk = torch.randn(256, H2, D2, generator=g).to(dt).to(cuda)
        vv = torch.randn(256, H2, D2, generator=g).to(dt).to(cuda)
        tab2 = ops.rope_table(256, D2, 10000.0, cuda)
        sc2 = ops.decode_attn_scratch(H2, D2, cuda)
        q2 = torch.randn(1, 3 * H2 * D2, generator=g).to(cuda)
        ka, va, kb, vb = kk.clone(), vv.clone(), kk.clone(), vv.clone()
        r2 = ops.llama_decode_attn(q2, ka, va, H2, D2, 200, 10000.0, D2 ** -0.5, table=tab2)
        g2 = ops.llama_decode_attn(q2, kb, vb, H2, D2, 200, 10000.0, D2 ** -0.5, table=tab2, scratch=sc2)
        assert torch.equal(ka, kb) and float((g2 - r2).abs().max()) < 2e-6 * max(1.0, float(r2.abs().max()))
    finally:
        hip_lib.ivlm_llama_decode_attn_splits(8)


@pytest.mark.parametrize("precision", ["f16", "default"])
def test_graph_decode_with_splitkv_attention_matches_one_block_kernel(hip_lib, cuda, precision):
    """A replayed decode graph with the opt-in split-KV attention (`decode_splitkv`) against eager steps on the one-block-per-head
    kernel: same argmax ids, hidden states and KV cache to fp32 summation order; two generations on one graph / scratch."""
    import torch

    from interactvlm_amd import llava, ops
    from interactvlm_amd import weights as Wt

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1003)
    w = _bf16_weights(Wt.llama_spec(lc))
    g = torch.Generator().manual_seed(5)
    T0, n_new = 150, 12
    emb = (torch.randn(T0, 512, generator=g) * 0.5).to(torch.bfloat16).float().to(cuda)
    toks = torch.randint(3, 1000, (n_new,), generator=g).to(torch.int32).to(cuda)
    llm_a = llava.Llama(w, lc, cuda, max_len=256)
    llm_a.set_precision(precision)
    llm_a.forward(emb, 0)
    hid_a, arg_a = [], []
    for s in range(n_new):
        h = llm_a.forward(llm_a.embed_ids(toks[s: s + 1]), T0 + s)
        hid_a.append(h)
        arg_a.append(int(ops.argmax(llm_a.logits(h))[0]))
    llm_b = llava.Llama(w, lc, cuda, max_len=256)
    llm_b.set_precision(precision)
    llm_b.decode_splitkv = True
    llm_b.decode_attn_parts = False  # (the default form - partials merged by the packed o_proj - has its own test below)
    llm_b.forward(emb, 0)
    dg = llm_b.decode_graph()
    assert llm_b._dec_scratch is not None
    for rep in range(2):
        dg["pos"].fill_(T0)
        dg["pos64"].fill_(T0)
        hid_b, arg_b = [], []
        for s in range(n_new):
            dg["tok"].copy_(toks[s: s + 1])
            dg["graph"].replay()
            hid_b.append(dg["hidden"].clone())
            arg_b.append(int(dg["nxt"][0]))
        assert _rel_err(torch.cat(hid_b), torch.cat(hid_a).float().cpu()) < 1e-5
        assert arg_a == arg_b
        # layer 0 appends rows computed from identical inputs: the same bits; deeper layers see the other summation order
        (ka, va), (kb, vb) = llm_a._caches(), llm_b._caches()
        assert torch.equal(ka[0, :T0 + n_new], kb[0, :T0 + n_new]) and torch.equal(va[0, :T0 + n_new], vb[0, :T0 + n_new])
        assert float((ka[:, :T0 + n_new].float() - kb[:, :T0 + n_new].float()).abs().max()) < 1e-2


def test_nonfinite_result_of_an_fp16_mode_is_recomputed_in_bf16(hip_lib, cuda, golden_dir):
    """fp16 operands have 5 exponent bits: weights that push an activation past 65504 (here gate / up projections scaled by 2^11, so
    that SiLU(gate) * up of the prefill overflows) make the default mode's contacts NaN.  evaluate() notices (one flag on the
    result), recomputes the call with bf16 operands (same arithmetic, fp32's exponent range), warns and marks the result; the
    unguarded model returns the NaNs; an in-range model is never touched by the guard."""
    import warnings

    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    bf = torch.bfloat16
    ic, im = images_clip.to(bf).to(cuda), images.to(bf).to(cuda)
    args = (ic, im, ids[None, :40], cams, [(1024, 1024)], [(1024, 1024)])
    kw = dict(forced_new_tokens=ids[40:].tolist())
    m0 = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an in-range model: no warning, no recomputation
        ok = m0.evaluate(*args, **kw)
    assert "recomputed_in_bf16" not in ok and bool(torch.isfinite(ok["pred_contact_3d"]).all())
    del m0
    w2 = dict(w)
    for n in ("gate_proj", "up_proj"):
        k = f"model.layers.0.mlp.{n}.weight"
        w2[k] = (w[k].float() * 2048.0).to(bf)
    m = M.InteractVLMForCausalLM(cfg, w2, cuda, lift_tables=tables)
    assert m.precision == "default" and m.nonfinite_guard
    m.nonfinite_guard = False
    raw = m.evaluate(*args, **kw)
    assert not bool(torch.isfinite(raw["pred_contact_3d"]).all())  # the premise: this model overflows fp16
    m.nonfinite_guard = True
    with pytest.warns(UserWarning, match="recomputed with bf16 operands"):
        out = m.evaluate(*args, **kw)
    assert out.get("recomputed_in_bf16") is True and m.precision == "default"
    assert bool(torch.isfinite(out["pred_contact_3d"]).all())
    with pytest.warns(UserWarning, match="recomputed with bf16 operands"):
        outs = m.evaluate_batch(ic.repeat(2, 1, 1, 1), im.repeat(2, 1, 1, 1, 1), [ids[:40], ids[:40]], [cams[0]] * 2,
                                [(1024, 1024)] * 2, [(1024, 1024)] * 2, forced_new_tokens=ids[40:].tolist())
    assert all(o.get("recomputed_in_bf16") and bool(torch.isfinite(o["pred_contact_3d"]).all()) for o in outs)
    m.set_precision("bf16")
    m.llm.decode_packed = False  # (the recomputation also decodes on the bf16 weights: fp32 activations with the full fp32 range)
    ref = m.evaluate(*args, **kw)
    assert torch.equal(out["pred_contact_3d"], ref["pred_contact_3d"]) and torch.equal(out["output_ids"], ref["output_ids"])
    assert float((outs[1]["pred_contact_3d"] - ref["pred_contact_3d"]).abs().max()) < 1e-3


@pytest.mark.parametrize("cache_dtype", ["bf16", "f16"])
def test_decode_attn_parts_merged_by_the_oproj_prologue(hip_lib, cuda, cache_dtype):
    """The default decode step's attention: four key ranges per head publish (o, max, sum) partials (ivlm_llama_decode_attn_parts) and the
    packed o_proj GEMV merges them while it stages its activation row (ivlm_gemv1_bf12m_parts).  Against the one-block attention +
    the packed GEMV on its output: the same appended cache rows, x + W_o a to fp32 summation order - at positions that leave ranges
    empty, fill exactly one tile, need several tiles, and past the slab (attention row = 0: the residual comes back unchanged)."""
    import torch

    from interactvlm_amd import ops

    H, D, Tmax = 8, 128, 2048
    hidden = H * D
    dt = torch.bfloat16 if cache_dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(21)
    kc0 = torch.randn(Tmax, H, D, generator=g).to(dt).to(cuda)
    vc0 = torch.randn(Tmax, H, D, generator=g).to(dt).to(cuda)
    tab = ops.rope_table(Tmax, D, 10000.0, cuda)
    wo = (torch.randn(hidden, hidden, generator=g) / hidden ** 0.5).bfloat16().to(cuda)
    wp = ops.PackedBf12(wo)
    assert wp.frag
    parts = torch.zeros(H * 4 * (D + 4), dtype=torch.float32, device=cuda)
    for pos in (0, 5, 95, 96, 330, 383, 384, 700, 1999, Tmax - 1):
        qkv = torch.randn(1, 3 * hidden, generator=g).to(cuda)
        res = torch.randn(1, hidden, generator=g).to(cuda)
        k1, v1, k2, v2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
        a = ops.llama_decode_attn(qkv, k1, v1, H, D, pos, 10000.0, D ** -0.5, table=tab)
        ref = ops.linear_bf12(a, wp, residual=res)
        p_arg = torch.tensor([pos], dtype=torch.int32, device=cuda) if pos % 2 else pos
        ops.llama_decode_attn_parts(qkv, k2, v2, H, D, p_arg, 10000.0, D ** -0.5, parts, table=tab)
        got = ops.linear_bf12(None, wp, residual=res, parts=(parts, D))
        assert torch.equal(k1, k2) and torch.equal(v1, v2), pos
        err = float((got - ref).abs().max())
        assert err < 3e-6 * max(1.0, float(ref.abs().max())), (pos, err)
    sk, sv = kc0[:64].clone(), vc0[:64].clone()
    res = torch.randn(1, hidden, generator=g).to(cuda)
    ops.llama_decode_attn_parts(torch.randn(1, 3 * hidden, generator=g).to(cuda), sk, sv, H, D,
                                torch.tensor([64], dtype=torch.int32, device=cuda), 10000.0, D ** -0.5, parts, table=tab)
    out = ops.linear_bf12(None, wp, residual=res, parts=(parts, D))
    assert torch.equal(out, res) and torch.equal(sk, kc0[:64]) and torch.equal(sv, vc0[:64])
