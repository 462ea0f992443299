"""Speculative greedy decoding on the GPU: the multi-token verify attention (ivlm_llama_verify_attn[_f16]) against a torch fp64
restatement and against the single-token kernel's cache appends, Llama.verify_step against k sequential decode steps, and
generate / evaluate with drafts on the toy model (same ids as the plain loop, no state left behind)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# batch-vs-single bound of the multi-row decode linears (the precision table: hi + lo operands, 2.6e-4)
BOUND_ROWS = 2.6e-4


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))


@pytest.mark.parametrize("cache_dtype", ["bf16", "f16"])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_verify_attn_vs_fp64_and_single_token_appends(hip_lib, cuda, cache_dtype, k):
    import torch

    from interactvlm_amd import ops

    H, D, Tmax = 8, 128, 300
    dt = torch.bfloat16 if cache_dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(11 + k)
    tab = ops.rope_table(Tmax, D, 10000.0, cuda)
    cos, sin = tab[0].double().cpu(), tab[1].double().cpu()
    for pos in (0, 37, 260, Tmax - 3):  # (the last: rows pos+3 .. pos+k-1 fall past the slab)
        qkv = torch.randn(k, 3 * H * D, generator=g).to(cuda)
        big_k = torch.randn(Tmax + 16, H, D, generator=g).to(dt).to(cuda)  # the slab + rows behind it that must stay untouched
        big_v = torch.randn(Tmax + 16, H, D, generator=g).to(dt).to(cuda)
        kc0, vc0 = big_k.clone(), big_v.clone()
        pos_dev = torch.tensor([pos], dtype=torch.int32, device=cuda)
        o = ops.llama_verify_attn(qkv, big_k[:Tmax], big_v[:Tmax], H, D, pos_dev, 10000.0, D ** -0.5, table=tab)
        kv = max(0, min(k, Tmax - pos))
        assert torch.equal(big_k[Tmax:], kc0[Tmax:]) and torch.equal(big_v[Tmax:], vc0[Tmax:])
        assert torch.equal(big_k[:pos], kc0[:pos]) and torch.equal(big_v[:pos], vc0[:pos])
        if kv < k:  # rows past the slab: zero output rows
            assert float(o[kv:].abs().max()) == 0.0
        # the appended rows are what k single-token decode steps append for the same qkv rows
        sk, sv = kc0[:Tmax].clone(), vc0[:Tmax].clone()
        for i in range(kv):
            ops.llama_decode_attn(qkv[i: i + 1].contiguous(), sk, sv, H, D, pos + i, 10000.0, D ** -0.5, table=tab)
        assert torch.equal(big_k[:Tmax], sk) and torch.equal(big_v[:Tmax], sv), (pos, k)
        # fp64 restatement: query i sees the cached rows, the new rows < i as cached, its own row unrounded
        rot = lambda t: torch.cat([-t[..., D // 2:], t[..., : D // 2]], -1)
        Kc, Vc = big_k[:Tmax].double().cpu(), big_v[:Tmax].double().cpu()
        for i in range(kv):
            p = pos + i
            x = qkv[i].double().cpu().view(3, H, D)
            c, s_ = torch.cat([cos[p], cos[p]]), torch.cat([sin[p], sin[p]])
            qr, kr = x[0] * c + rot(x[0]) * s_, x[1] * c + rot(x[1]) * s_
            K_ = torch.cat([Kc[:p], kr[None]], 0)
            V_ = torch.cat([Vc[:p], x[2][None]], 0)
            a = torch.softmax(torch.einsum("hd,thd->ht", qr, K_) * D ** -0.5, -1)
            ref = torch.einsum("ht,thd->hd", a, V_).reshape(-1)
            err = float((o[i].double().cpu() - ref).abs().max())
            assert err < 2e-5, (pos, k, i, err)


@pytest.mark.parametrize("precision", ["f16", "default"])
def test_verify_step_equals_sequential_decode_steps(hip_lib, cuda, precision):
    """verify_step on k tokens vs k sequential _decode_step calls: hidden rows within the batch-vs-single bound (the multi-row
    linears take hi + lo operands, the single-row ones exact products); the cache rows agree to that bound plus one rounding of
    the storage type - bit for bit where the qkv rows are equal (the test above), with qkv rows ~1e-5 apart an element that lies
    near a rounding boundary of the cache type lands on the other side."""
    import torch

    from interactvlm_amd import llava
    from interactvlm_amd import weights as Wt

    lc = Wt.LlamaCfg(hidden=512, layers=3, heads=4, inter=1024, vocab=1003)
    w = {k_: v.to(torch.bfloat16).float() for k_, v in Wt.synth_weights(Wt.llama_spec(lc), 5).items()}
    g = torch.Generator().manual_seed(29)
    T0 = 37
    emb = (torch.randn(T0, 512, generator=g) * 0.5).to(torch.bfloat16).float().to(cuda)
    llm = llava.Llama(w, lc, cuda, max_len=96)
    llm.set_precision(precision)
    llm.prepare()
    llm.release_unused()
    before = llm.resident_bytes()
    for k in (1, 4, 9, 16):
        toks = torch.randint(3, 1000, (k,), generator=g).to(torch.int32).to(cuda)
        llm.forward(emb, 0)
        seq = torch.cat([llm._decode_step(llm.embed_ids(toks[i: i + 1]), T0 + i) for i in range(k)])
        kc_s, vc_s = [t[:, T0: T0 + k].float().clone() for t in llm._caches()]
        llm.forward(emb, 0)
        h = llm.verify_step(llm.embed_ids(toks), torch.tensor([T0], dtype=torch.int32, device=cuda))
        kc_v, vc_v = [t[:, T0: T0 + k].float() for t in llm._caches()]
        e = _rel(h, seq)
        print(f"\n[verify_step {precision} k={k}] hidden rel err {e:.2e}")
        assert e < BOUND_ROWS, (k, e)
        ulp = 2.0 ** -7 if precision == "default" else 2.0 ** -10
        for a_, b_ in ((kc_v, kc_s), (vc_v, vc_s)):  # (one storage rounding on top of the rows' own difference)
            same = float((a_ == b_).float().mean())
            print(f"[verify_step {precision} k={k}] cache rows bit-identical: {same:.4f}")
            assert bool(((a_ - b_).abs() <= ulp * b_.abs() + BOUND_ROWS * b_.abs().max()).all()), k
            assert same > 0.9, (k, same)
    assert llm.resident_bytes() == before


class _Prop:
    """proposes the greedy continuation, its ids from the j-th on replaced by wrong ones (j = 0: all wrong; None: all right)"""

    def __init__(self, greedy, vocab, j=None, n=None):
        self.greedy, self.vocab, self.j, self.n = greedy, vocab, j, n

    def propose(self, ids, k):
        cont = self.greedy[len(ids): len(ids) + (k - 1 if self.n is None else min(self.n, k - 1))]
        if self.j is not None:
            cont = cont[: self.j] + [(t + 1) % self.vocab for t in cont[self.j:]]
        return cont


def _expected_pattern(n_new, prop_len, j):
    """(proposed, accepted) per verify pass of the loop for a draft of prop_len ids per round, right for its first j"""
    out, have = [], 1
    while have < n_new:
        m = min(prop_len, 15, n_new - have - 1)
        if m == 0:
            have += 1
            continue
        n = m if j is None else min(j, m)
        out.append((m, n))
        have += n + 1
    return out


def _toy_model(golden_dir, cuda):
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt
    from test_model_gpu import _toy

    d, cfg, ids, images_clip, images, cams, tables = _toy(golden_dir)
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    return m, cfg, ids, images_clip.to(torch.bfloat16).to(cuda), images.to(torch.bfloat16).to(cuda), cams


def test_generate_with_drafts_equals_plain_generate(hip_lib, cuda, golden_dir):
    import torch

    torch.set_grad_enabled(False)
    m, cfg, ids, ic, im, cams = _toy_model(golden_dir, cuda)
    prompt = ids[:40][None]
    L = prompt.shape[1]
    n_new = 20
    V = cfg.llama.vocab
    for graph in (True, False):
        m.graph_decode = graph
        plain_ids, plain_h = m.generate(ic, prompt, max_new_tokens=n_new, eos_token_id=-1)
        greedy = plain_ids[0, L:].tolist()
        assert len(greedy) == n_new
        cases = [(None, None), (0, 15), (0, 3), (2, None), (5, 6)]  # (right for j ids, ids per proposal)
        for j, n in cases:
            got_ids, got_h = m.generate(ic, prompt, max_new_tokens=n_new, eos_token_id=-1, draft=_Prop(greedy, V, j, n))
            assert torch.equal(got_ids, plain_ids), (graph, j, n)
            assert got_h.shape == plain_h.shape
            e = _rel(got_h, plain_h)
            assert e < BOUND_ROWS, (graph, j, n, e)
            assert m.last_spec["pattern"] == _expected_pattern(n_new, 15 if n is None else n, j), (graph, j, n, m.last_spec)
            assert len(m.last_argmax) == n_new
        # EOS inside an accepted draft: the loop stops on it; the hidden rows are the plain loop's count
        eos = greedy[7]
        first = greedy.index(eos)
        e_ids, e_h = m.generate(ic, prompt, max_new_tokens=n_new, eos_token_id=eos, draft=_Prop(greedy, V))
        assert e_ids[0, L:].tolist() == greedy[: first + 1] and m.last_spec["passes"] == 1
        assert e_h.shape[0] == plain_h.shape[0] - (n_new - 1 - first)
        # nothing leaks: a plain generate after the speculative calls is bit-identical to the one before them
        again_ids, again_h = m.generate(ic, prompt, max_new_tokens=n_new, eos_token_id=-1)
        assert torch.equal(again_ids, plain_ids) and torch.equal(again_h, plain_h)
    # the verify graphs sit in the decode-graph cache and leave with it (fp8 / precision events drop every entry)
    assert any(k.verify for k in m.llm._graphs)
    m.llm._drop_graphs(lambda k: k.verify)
    assert not any(k.verify for k in m.llm._graphs)


def test_evaluate_with_an_accepted_draft(hip_lib, cuda, golden_dir):
    import torch

    from interactvlm_amd.speculative import Drafter

    torch.set_grad_enabled(False)
    m, cfg, ids, ic, im, cams = _toy_model(golden_dir, cuda)
    prompt = ids[:40][None]
    L = prompt.shape[1]
    n_new = 12
    greedy = m.generate(ic, prompt, max_new_tokens=n_new, eos_token_id=-1)[0][0, L:].tolist()
    m.seg_token_idx = greedy[6]  # (random weights never emit [SEG]: an id the model does emit stands in for it)
    before = m.resident_weight_bytes()
    sz = [(1024, 1024)]
    plain = m.evaluate(ic, im, prompt, cams, sz, sz, max_new_tokens=n_new, eos_token_id=-1)
    spec = m.evaluate(ic, im, prompt, cams, sz, sz, max_new_tokens=n_new, eos_token_id=-1, draft=Drafter([greedy]))
    assert m.last_spec["passes"] >= 1 and m.last_spec["accepted"] == m.last_spec["proposed"]
    assert torch.equal(spec["output_ids"], plain["output_ids"])
    assert plain["pred_contact_3d"] is not None and plain["pred_contact_3d"].shape == (1, 6890)
    e = float((spec["pred_contact_3d"] - plain["pred_contact_3d"]).abs().max())
    print(f"\n[evaluate with draft] max|dp| = {e:.2e}")
    assert e < 1e-3
    assert m.resident_weight_bytes() == before


def test_parity_mode_falls_back_to_the_plain_loop(hip_lib, cuda):
    """"parity" caches K / V as hi + lo planes, which the verify attention does not read: generate(draft=) runs the plain loop there
    (on the structurally complete tiny configuration - the parity attention needs the real head dims)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import synth, synthetic
    from interactvlm_amd import weights as Wt

    torch.set_grad_enabled(False)
    cfg = synthetic.config_tiny()
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    ids, _ = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    ic, _ = synthetic.images(cfg, cuda)
    m.set_precision("parity")
    assert not m.llm.verify_supported()
    plain = m.generate(ic, ids, max_new_tokens=6, eos_token_id=-1)
    greedy = plain[0][0, ids.shape[1]:].tolist()
    got = m.generate(ic, ids, max_new_tokens=6, eos_token_id=-1, draft=_Prop(greedy, cfg.llama.vocab))
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and m.last_spec is None
    assert np.isfinite(got[1].float().cpu().numpy()).all()
    m.set_precision("default")  # ... and the default mode of the same model speculates
    assert m.llm.verify_supported()
    plain = m.generate(ic, ids, max_new_tokens=6, eos_token_id=-1)
    greedy = plain[0][0, ids.shape[1]:].tolist()
    got = m.generate(ic, ids, max_new_tokens=6, eos_token_id=-1, draft=_Prop(greedy, cfg.llama.vocab))
    assert torch.equal(got[0], plain[0]) and m.last_spec["passes"] == 1
