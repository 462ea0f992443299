"""Several questions about ONE picture share the prompt prefix (generate_batch / evaluate_batch share_prefix=True): the decode
attention kernel that reads the shared rows once for all sequences, the prefill that computes them once, and the public path."""
import pytest

pytestmark = pytest.mark.gpu

H, D, TMAX = 8, 128, 96


def _positions(B, P):
    """different per sequence; one at P (own range = the new row only), the last at Tmax (skipped)"""
    return [P] + [P + 1 + (7 * i) % (TMAX - P - 1) for i in range(1, B - 1)] + [TMAX]


def _state(B, P, cache_dtype, cuda, seed=3):
    import torch

    from interactvlm_amd import ops

    dt = torch.float16 if cache_dtype == "f16" else torch.bfloat16
    g = torch.Generator().manual_seed(seed + B + P)
    q32 = torch.randn(B, 3 * H * D, generator=g).to(cuda)
    kc = torch.randn(B, TMAX, H, D, generator=g).to(dt).to(cuda)
    vc = torch.randn(B, TMAX, H, D, generator=g).to(dt).to(cuda)
    kc[1:, :P] = kc[:1, :P]  # what the product path guarantees: every slab holds the prefix rows
    vc[1:, :P] = vc[:1, :P]
    pos = _positions(B, P)
    return q32, kc, vc, pos, torch.tensor(pos, dtype=torch.int32, device=cuda), ops.rope_table(TMAX, D, 10000.0, cuda), dt


@pytest.mark.parametrize("cache_dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", [17, 64])
@pytest.mark.parametrize("B", [2, 5, 16])
def test_prefix_kernel_vs_torch_fp64(hip_lib, cuda, B, P, cache_dtype):
    """ivlm_llama_decode_attn_batch_prefix[_f16] against torch fp64 on fp32 q, the cache's 16-bit history and the exact new row
    (inputs, reference and the 2e-5 bound of test_decode_attn_batch_equals_per_sequence, the kernel this one stands beside)."""
    import torch

    from interactvlm_amd import ops

    q32, kc, vc, pos, pos_dev, tab, dt = _state(B, P, cache_dtype, cuda)
    pre = torch.tensor([P], dtype=torch.int32, device=cuda)
    kc2, vc2 = kc.clone(), vc.clone()
    got = ops.llama_decode_attn_batch_prefix(q32, kc2, vc2, H, D, pos_dev, pre, 10000.0, D ** -0.5, table=tab, host_check=(pos, P))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (B, H * D)
    # the sequence at Tmax: a zero row, its slab untouched
    assert float(got[B - 1].abs().max()) == 0.0
    assert torch.equal(kc2[B - 1], kc[B - 1]) and torch.equal(vc2[B - 1], vc[B - 1])
    cos, sin = tab[0].double().cpu(), tab[1].double().cpu()
    worst = 0.0
    for b in range(B - 1):
        p = pos[b]
        x = q32[b].double().cpu().view(3, H, D)
        c, s_ = torch.cat([cos[p], cos[p]]), torch.cat([sin[p], sin[p]])
        rot = lambda t: torch.cat([-t[..., D // 2:], t[..., : D // 2]], -1)
        qr, kr = x[0] * c + rot(x[0]) * s_, x[1] * c + rot(x[1]) * s_
        K_ = torch.cat([kc[b, :p].double().cpu(), kr[None]], 0)  # [p+1, H, D]: 16-bit history + exact new row
        V_ = torch.cat([vc[b, :p].double().cpu(), x[2][None]], 0)
        a = torch.softmax(torch.einsum("hd,thd->ht", qr, K_) * D ** -0.5, -1)
        ref = torch.einsum("ht,thd->hd", a, V_).reshape(-1)
        e = float((got[b].double().cpu() - ref).abs().max())
        worst = max(worst, e)
        assert e < 2e-5, (b, p, e)
        # the new row was appended (rounded to the cache's dtype), every other row of the slab - its neighbours' too - untouched
        assert float((kc2[b, p].double().cpu() - kr).abs().max()) <= 2.0 ** -8 * float(kr.abs().max())
        assert torch.equal(vc2[b, p], x[2].to(dt).to(cuda))
        for new, old in ((kc2, kc), (vc2, vc)):
            rest = new[b].clone()
            rest[p] = old[b, p]
            assert torch.equal(rest, old[b])
    print(f"\n[prefix kernel B={B} P={P} {cache_dtype}] max|o - fp64| = {worst:.2e}")
    # the prefix is read from slab 0 only: other contents in rows [0, P) of slabs 1 .. B-1 do not change the output
    kc3, vc3 = kc.clone(), vc.clone()
    kc3[1:, :P] = 7.0
    vc3[1:, :P] = 7.0
    got3 = ops.llama_decode_attn_batch_prefix(q32, kc3, vc3, H, D, pos_dev, pre, 10000.0, D ** -0.5, table=tab)
    assert torch.equal(got3, got)
    # a launch is reproducible (fixed merge order)
    kc4, vc4 = kc.clone(), vc.clone()
    assert torch.equal(ops.llama_decode_attn_batch_prefix(q32, kc4, vc4, H, D, pos_dev, pre, 10000.0, D ** -0.5, table=tab), got)


@pytest.mark.parametrize("cache_dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,P", [(2, 17), (5, 64), (16, 64), (16, 17)])
def test_prefix_kernel_and_plain_batch_kernel_on_the_same_state(hip_lib, cuda, B, P, cache_dtype):
    """On identical caches the outputs differ by the fp32 summation order only (2e-5) and the appended K / V rows are bit-identical."""
    import torch

    from interactvlm_amd import ops

    q32, kc, vc, pos, pos_dev, tab, dt = _state(B, P, cache_dtype, cuda, seed=11)
    pre = torch.tensor([P], dtype=torch.int32, device=cuda)
    kc1, vc1, kc2, vc2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    plain = ops.llama_decode_attn_batch(q32, kc1, vc1, H, D, pos_dev, 10000.0, D ** -0.5, table=tab)
    got = ops.llama_decode_attn_batch_prefix(q32, kc2, vc2, H, D, pos_dev, pre, 10000.0, D ** -0.5, table=tab)
    e = float((got - plain).abs().max())
    print(f"\n[prefix vs plain B={B} P={P} {cache_dtype}] max|do| = {e:.2e}")
    assert e < 2e-5
    assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    assert not torch.equal(kc2, kc)  # (rows were appended)


def test_prefix_kernel_rejects_what_it_does_not_support(hip_lib, cuda):
    import torch

    from interactvlm_amd import _lib, ops

    tab = ops.rope_table(TMAX, D, 10000.0, cuda)
    pre = torch.tensor([20], dtype=torch.int32, device=cuda)

    def call(B, H_, D_, table=tab):
        q = torch.zeros(B, 3 * H_ * D_, device=cuda)
        kc = torch.zeros(B, TMAX, H_, D_, dtype=torch.bfloat16, device=cuda)
        pos = torch.full((B,), 30, dtype=torch.int32, device=cuda)
        return ops.llama_decode_attn_batch_prefix(q, kc, kc.clone(), H_, D_, pos, pre, 10000.0, D_ ** -0.5, table=table)

    for bad in ((17, H, D, tab), (2, 2, 256, None), (2, 2, 72, None)):  # B > 16, D > 128, D % 16 != 0
        with pytest.raises(_lib.IvlmError, match="unsupported"):
            call(*bad)
    torch.cuda.synchronize()
    assert float(call(2, H, D).abs().max()) == 0.0  # (zero V rows: the valid call still runs)
    with pytest.raises(AssertionError):  # a sequence inside the prefix: refused on the host where the caller has the numbers
        q = torch.zeros(2, 3 * H * D, device=cuda)
        kc = torch.zeros(2, TMAX, H, D, dtype=torch.bfloat16, device=cuda)
        ops.llama_decode_attn_batch_prefix(q, kc, kc.clone(), H, D, torch.tensor([30, 19], dtype=torch.int32, device=cuda), pre, 10000.0,
                                           D ** -0.5, table=tab, host_check=([30, 19], 20))
    # what the decode-attention wrappers check alike before they launch, one input per check: a position tensor that is not int32, K and
    # V caches of different dtypes, a RoPE table shorter than the cache
    q = torch.zeros(2, 3 * H * D, device=cuda)
    kc = torch.zeros(2, TMAX, H, D, dtype=torch.bfloat16, device=cuda)
    pos = torch.tensor([30, 40], dtype=torch.int32, device=cuda)
    short = tuple(t[: TMAX - 1] for t in tab)
    rest = (10000.0, D ** -0.5)
    for bad in (lambda: ops.llama_decode_attn_batch_prefix(q, kc, kc.clone(), H, D, pos.long(), pre, *rest, table=tab),
                lambda: ops.llama_decode_attn_batch_prefix(q, kc, kc.half(), H, D, pos, pre, *rest, table=tab),
                lambda: ops.llama_decode_attn_batch_prefix(q, kc, kc.clone(), H, D, pos, pre, *rest, table=short),
                lambda: ops.llama_decode_attn_batch(q, kc, kc.clone(), H, D, pos.long(), *rest, table=tab),
                lambda: ops.llama_decode_attn(q[:1], kc[0], kc[1], H, D, pos[:1].long(), *rest, table=tab),
                lambda: ops.llama_verify_attn(q, kc[0], kc[1].half(), H, D, pos[:1], *rest, table=tab),
                lambda: ops.llama_verify_attn(q, kc[0], kc[1], H, D, pos[:1], *rest, table=short)):
        with pytest.raises(AssertionError):
            bad()
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["default", "f16"])
def test_shared_prefix_prefill_equals_packed_prefill(hip_lib, cuda, precision):
    """Llama.forward_shared_prefix (the 24 shared rows once into slab 0, copied to the other slabs, then the three suffixes as packed
    segments at position 24) against forward_packed on a second set of slabs: the hidden rows and every written cache row.
    Observed on an MI355X: bit for bit in both modes, as packed == per-sequence is at this size."""
    import torch

    from interactvlm_amd import llava
    from interactvlm_amd import weights as Wt
    from test_model_gpu import _bf16_weights

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1003)
    w = _bf16_weights(Wt.llama_spec(lc))
    g = torch.Generator().manual_seed(31)
    P, lens = 24, (40, 33, 47)
    head = (torch.randn(P, 512, generator=g) * 0.5).to(torch.bfloat16).float()
    xs = [torch.cat([head, (torch.randn(T - P, 512, generator=g) * 0.5).to(torch.bfloat16).float()]).to(cuda) for T in lens]
    llm = llava.Llama(w, lc, cuda, max_len=64)
    llm.set_precision(precision)
    dt = torch.float16 if precision == "f16" else torch.bfloat16
    slab_s, slab_p = ([torch.zeros(lc.layers, len(lens), 64, 4, 128, dtype=dt, device=cuda) for _ in range(2)] for _ in range(2))
    hs = llm.forward_shared_prefix(xs, P, slab_s[0], slab_s[1])
    hp = llm.forward_packed(xs, slab_p[0], slab_p[1])
    for b, T in enumerate(lens):
        dk = max(float((ts[:, b, :T].float() - tp[:, b, :T].float()).abs().max()) for ts, tp in zip(slab_s, slab_p))
        print(f"\n[{precision}] prompt {b} (T = {T}): max|dh| = {float((hs[b] - hp[b]).abs().max()):.3e}, max|d cache| = {dk:.3e}")
    for b, T in enumerate(lens):
        assert hs[b].shape == (T, 512) and torch.equal(hs[b], hp[b])
        for ts, tp in zip(slab_s, slab_p):
            assert torch.equal(ts[:, b, :T], tp[:, b, :T])
    with pytest.raises(Exception):
        llm.forward_shared_prefix(xs, 16, slab_s[0], slab_s[1])  # (the prefix pass is a tile GEMM: P > 16)


def _one_picture_case(golden_dir, cuda):
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth
    from interactvlm_amd import weights as Wt
    from test_model_gpu import _toy

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    bf = torch.bfloat16
    B = 3
    ic = torch.from_numpy(synth.synth_normal("eb/images_clip", (B, 3, 224, 224), 1.0, 0)).to(bf).to(cuda)
    im = torch.from_numpy(synth.synth_normal("eb/images", (B, 4, 3, 1024, 1024), 1.0, 0)).to(bf).to(cuda)
    # three questions about one picture: the same first 30 ids (image at index 11), different tails of different lengths
    prompts = [ids[:40].clone(), torch.cat([ids[:30], ids[34:40]]), torch.cat([ids[:30], ids[31:40]])]
    forced = [ids[40:].tolist(), ids[40:].tolist(), ids[40: len(ids) - 2].tolist() + [int(ids[-1])]]
    return m, ic, im, prompts, forced, [cams[0]] * B, [(1024, 1024)] * B


@pytest.mark.parametrize("graph", [True, False])
def test_evaluate_batch_share_prefix_equals_the_plain_path(hip_lib, cuda, golden_dir, graph, monkeypatch):
    """evaluate_batch / generate_batch with share_prefix=True against share_prefix=False for three questions about one picture:
    same ids, contacts within the 1e-3 that evaluate_batch is held to against evaluate; the captured step is reused; where
    nothing can be shared (one picture per prompt) the flag changes nothing, bit for bit."""
    import torch

    from interactvlm_amd import decoding, ops

    m, ic, im, prompts, forced, cam_b, sizes = _one_picture_case(golden_dir, cuda)
    m.graph_decode = graph
    B = len(prompts)
    P = decoding.shared_prefix_len([p.tolist() for p in prompts], True, m.precision)
    assert P == 30 - 1 + 256
    calls = []
    real = ops.llama_decode_attn_batch_prefix
    monkeypatch.setattr(ops, "llama_decode_attn_batch_prefix", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for mode in ("default", "bf16"):
        m.set_precision(mode)
        mine = lambda: [k for k in m.llm._graphs if k.prefix and k.precision == m.llm.precision]
        n0 = len(calls)
        plain = m.evaluate_batch(ic[:1], im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced)
        assert len(calls) == n0 and not mine()  # (the default leaves every launch and graph as it was)
        outs = m.evaluate_batch(ic[:1], im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced, share_prefix=True)
        assert len(calls) > n0  # (the new kernel ran: eagerly, or while its graph was captured)
        assert sorted(outs[0]) == sorted(plain[0])
        for b in range(B):
            assert torch.equal(outs[b]["output_ids"], plain[b]["output_ids"])
            e = float((outs[b]["pred_contact_3d"] - plain[b]["pred_contact_3d"]).abs().max())
            em = float((outs[b]["pred_masks"][0] - plain[b]["pred_masks"][0]).abs().max())
            print(f"\n[share_prefix {mode} graph={graph}] question {b}: max|dp| = {e:.2e}, max|dmask| = {em:.3e}")
            assert outs[b]["pred_contact_3d"].shape == (1, 6890)
            assert e < 1e-3
        # a second call reuses the captured graph (and the cache slabs) and returns the same contacts
        keys = mine()
        assert len(keys) == (1 if graph else 0)
        st = m.llm._graphs[keys[0]] if graph else None
        n = len(calls)
        outs2 = m.evaluate_batch(ic[:1], im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced, share_prefix=True)
        for b in range(B):
            assert torch.equal(outs2[b]["pred_contact_3d"], outs[b]["pred_contact_3d"])
        if graph:
            assert mine() == keys and m.llm._graphs[keys[0]] is st and len(calls) == n
        # the deferred form takes the flag too
        outs3 = m.evaluate_batch(ic[:1], im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced, share_prefix=True, deferred=True)()
        for b in range(B):
            assert torch.equal(outs3[b]["pred_contact_3d"], outs[b]["pred_contact_3d"])
        # free-running greedy search: the same ids as the unshared path
        free0 = m.generate_batch(ic[:1], prompts, max_new_tokens=8, eos_token_id=-1)
        free1 = m.generate_batch(ic[:1], prompts, max_new_tokens=8, eos_token_id=-1, share_prefix=True)
        for b in range(B):
            n_ = min(free0[b][0].shape[1], free1[b][0].shape[1])
            assert n_ == prompts[b].numel() + 8 and torch.equal(free0[b][0][0, :n_], free1[b][0][0, :n_])
    # nothing to share: one picture per prompt -> exactly the plain path
    m.set_precision("default")
    n = len(calls)
    a0 = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced)
    a1 = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, forced_new_tokens=forced, share_prefix=True)
    assert len(calls) == n
    for b in range(B):
        assert torch.equal(a0[b]["output_ids"], a1[b]["output_ids"])
        assert torch.equal(a0[b]["pred_contact_3d"], a1[b]["pred_contact_3d"])
        assert torch.equal(a0[b]["pred_masks"][0], a1[b]["pred_masks"][0])


def test_share_prefix_in_the_parity_mode_is_the_plain_path(hip_lib, cuda, monkeypatch):
    """set_precision("parity") keeps hi + lo cache planes: share_prefix=True runs the plain path and returns exactly what
    share_prefix=False returns (the structurally complete tiny configuration, two questions about one picture)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import ops, synth, synthetic
    from interactvlm_amd import weights as Wt

    cfg = synthetic.config_tiny()
    w = {k: v.to(torch.bfloat16).float() for k, v in Wt.synth_weights(Wt.ivlm_spec(cfg)).items()}
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=52, n_answer=8)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    other = ids[0].clone()
    other[40:] = (other[40:] + 7) % 31000
    prompts, im2 = [ids[0], other[:49]], torch.cat([im, im])
    args = (ic, im2, prompts, [cams[0]] * 2, [(1024, 1024)] * 2, [(1024, 1024)] * 2)
    calls = []
    real = ops.llama_decode_attn_batch_prefix
    monkeypatch.setattr(ops, "llama_decode_attn_batch_prefix", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m.set_precision("parity")
    b0 = m.evaluate_batch(*args, forced_new_tokens=forced)
    b1 = m.evaluate_batch(*args, forced_new_tokens=forced, share_prefix=True)
    assert not calls
    for x0, x1 in zip(b0, b1):
        assert torch.equal(x0["output_ids"], x1["output_ids"]) and torch.equal(x0["pred_contact_3d"], x1["pred_contact_3d"])
        assert torch.equal(x0["pred_masks"][0], x1["pred_masks"][0])
    # (the same prompts do share their prefix in a mode that supports it)
    m.set_precision("default")
    c1 = m.evaluate_batch(*args, forced_new_tokens=forced, share_prefix=True)
    assert calls
    for x0, x1 in zip(b0, c1):
        assert torch.equal(x0["output_ids"], x1["output_ids"])
