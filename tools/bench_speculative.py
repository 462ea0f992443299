#!/usr/bin/env python3
"""Speculative greedy decoding at 7B (or 13B) shapes on synthetic weights: what a verify pass costs and what a draft buys.
    python tools/bench_speculative.py [--model 13b] [--out profiles/speculative_7b.json]

Reports plain free-running ms per token, verify-pass ms for k = 2, 4, 8, 16 (next to the batched decode step of k sequences it is
built from, and the two attention kernels alone), a 24-token generation with (a) the plain loop, (b) a draft equal to the model's own
greedy output, (c) a draft that is always wrong and always proposed, (d) a template bank that never matches, and batch-1 evaluate()
in images/s, plain and with the 100 %-accepted draft.  Random weights never emit [SEG]: the id the model emits at answer position 22
stands in for it (model.seg_token_idx), so evaluate() runs its SAM mask decoder and lift as on the headline schedule."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Fixed:
    """proposes ``n`` ids that the model never emits next (its own continuation + 1), every round"""

    def __init__(self, greedy, n, vocab):
        self.greedy, self.n, self.vocab = greedy, n, vocab

    def propose(self, ids, k):
        return [(self.greedy[min(len(ids) + j, len(self.greedy) - 1)] + 1) % self.vocab for j in range(min(self.n, k - 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b")
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from interactvlm_amd import model as M
    from interactvlm_amd import ops, synthetic
    from interactvlm_amd.speculative import Drafter

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = {"7b": synthetic.config_7b, "13b": synthetic.config_13b, "tiny": synthetic.config_tiny}[a.model]()
    weights = synthetic.device_weights(cfg, dev, seed=0)
    vid, bary = synthetic.body_lift_tables(dev)
    model = M.InteractVLMForCausalLM(cfg, weights, dev, lift_tables=(vid, bary))
    del weights
    llm = model.llm
    ids, _ = synthetic.prompt_ids(cfg)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, dev)
    S = cfg.sam.img_size
    n = a.tokens
    sync = torch.cuda.synchronize

    def wall(fn, reps=a.reps):
        fn()
        sync()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        return (time.perf_counter() - t) / reps * 1e3

    def gen(**kw):
        return model.generate(ic, ids, max_new_tokens=n, eos_token_id=-1, **kw)

    out_ids, hid = gen()
    greedy = out_ids[0, ids.shape[1]:].tolist()
    T0 = hid.shape[0] - (n - 1)  # prefill positions (the prompt with its image features)
    res = {"model": a.model, "tokens": n, "prefill_positions": T0, "graphs": bool(model.graph_decode)}
    t_pre = wall(lambda: model.generate(ic, ids, max_new_tokens=1, eos_token_id=-1))
    t_plain = wall(gen)
    res["ms_clip_prefill_first_id"] = round(t_pre, 3)
    res["plain_ms_per_token"] = round((t_plain - t_pre) / (n - 1), 4)

    # ---- one verify pass of k rows (graph replay at position T0), the batched step of k sequences, the attention kernels alone
    model.generate(ic, ids, max_new_tokens=1, eos_token_id=-1)  # (the prompt's K / V rows in the cache)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def replay_ms(st, reps=20, pos=T0):
        st["pos"].fill_(pos)
        st["graph"].replay()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(reps):
            st["pos"].fill_(pos)
            st["graph"].replay()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    H, D = cfg.llama.heads, cfg.llama.hidden // cfg.llama.heads
    kc, vc = llm._caches()
    verify, batched, attn = {}, {}, {}
    pos_dev = torch.full((1,), T0, dtype=torch.int32, device=dev)
    for k in (2, 4, 8, 16):
        st = llm.verify_graph(k)
        st["ids"].copy_(torch.tensor(greedy[:k], dtype=torch.int32))
        st["nd"].fill_(k - 1)
        verify[k] = round(replay_ms(st), 4)
        qkv = torch.randn(k, 3 * H * D, device=dev)
        f = lambda: ops.llama_verify_attn(qkv, kc[0], vc[0], H, D, pos_dev, cfg.llama.theta, D ** -0.5, table=llm.rope)
        f()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(50):
            f()
        e1.record()
        sync()
        attn[k] = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
    q1 = torch.randn(1, 3 * H * D, device=dev)
    g = lambda: ops.llama_decode_attn(q1, kc[0], vc[0], H, D, pos_dev, cfg.llama.theta, D ** -0.5, table=llm.rope)
    g()
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(50):
        g()
    e1.record()
    sync()
    attn_1 = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
    for k in (2, 4, 8, 16):
        dgb = llm.decode_graph_batch(k)
        dgb["pos"].fill_(T0)
        dgb["graph"].replay()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(20):
            dgb["pos"].fill_(T0)
            dgb["graph"].replay()
        e1.record()
        sync()
        batched[k] = round(e0.elapsed_time(e1) / 20, 4)
    P = res["plain_ms_per_token"]
    res["verify_pass_ms"] = verify
    res["batched_step_ms_same_rows"] = batched
    res["attention_us_per_layer"] = {"verify": attn, "single_token_decode": attn_1, "positions": T0}
    res["break_even"] = {k: {"accepted_per_pass": round(verify[k] / P - 1, 3),
                             "acceptance_rate": round(max(0.0, verify[k] / P - 1) / (k - 1), 3)} for k in verify}

    # ---- 24-token generations: (a) plain, (b) the model's own output, (c) always wrong, (d) a bank that never matches
    runs = {}

    def spec(name, make_draft):
        out = [None]

        def f():
            out[0] = gen(draft=make_draft())
        ms = wall(f)
        runs[name] = {"ids_equal_plain": out[0][0][0, ids.shape[1]:].tolist() == greedy, "ms": round(ms, 3), "ms_decode": round(ms - t_pre, 3), "passes": model.last_spec["passes"],
                      "plain_steps": model.last_spec["plain_steps"], "proposed": model.last_spec["proposed"],
                      "accepted": model.last_spec["accepted"]}

    runs["a_plain"] = {"ms": round(t_plain, 3), "ms_decode": round(t_plain - t_pre, 3)}
    spec("b_own_output", lambda: Drafter([greedy]))
    spec("c_always_wrong_15", lambda: _Fixed(greedy, 15, cfg.llama.vocab))
    spec("c_always_wrong_3", lambda: _Fixed(greedy, 3, cfg.llama.vocab))
    never = [[(t + 7) % cfg.llama.vocab for t in greedy[:6]], [(t + 11) % cfg.llama.vocab for t in greedy[6:12]]]
    spec("d_never_matches", lambda: Drafter(never))
    res["generate_24"] = runs

    # ---- batch-1 evaluate, free-running, plain and with the 100 %-accepted draft
    model.seg_token_idx = greedy[min(22, n - 2)]
    ev_plain = lambda: model.evaluate(ic, im, ids, cams, [(S, S)], [(S, S)], contact_type="hcontact", max_new_tokens=n, eos_token_id=-1)
    ev_spec = lambda: model.evaluate(ic, im, ids, cams, [(S, S)], [(S, S)], contact_type="hcontact", max_new_tokens=n, eos_token_id=-1,
                                     draft=Drafter([greedy]))
    o1, o2 = ev_plain(), ev_spec()
    dp = float((o1["pred_contact_3d"] - o2["pred_contact_3d"]).abs().max())
    t1, t2 = wall(ev_plain), wall(ev_spec)
    res["evaluate_b1"] = {"plain_images_per_s": round(1e3 / t1, 3), "plain_ms": round(t1, 3),
                          "draft_images_per_s": round(1e3 / t2, 3), "draft_ms": round(t2, 3), "max_abs_dcontact": dp,
                          "ids_equal": bool(torch.equal(o1["output_ids"], o2["output_ids"])),
                          "note": "free-running, max_new_tokens = 24, the id emitted at answer position 22 as [SEG]"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
