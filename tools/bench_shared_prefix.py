#!/usr/bin/env python3
"""K questions about ONE picture at 7B (or 13B) shapes on synthetic weights: what sharing the prompt prefix buys.
    python tools/bench_shared_prefix.py [--model 13b] [--out profiles/shared_prefix_7b.json]

Prompts: the 75-id headline prompt (image placeholder at index 36) and K copies that differ in their last 10 ids; 24 forced answer
ids each.  Per K in 2, 4, 8, 16 the whole ``generate_batch`` call is timed with share_prefix=False and True ALTERNATELY in one
process (``--pairs`` pairs after a warm-up pair; median and min-max spread of each), and next to it the pieces: the prefill alone
(forward_packed against forward_shared_prefix, and the broadcast copy of the prefix rows on its own), one captured decode step,
and the decode attention of one layer from kernel-attached events (ivlm_profile_launches), plain kernel against prefix kernel on
the same cache state.  The unshared leg is the path share_prefix=False takes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b")
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from interactvlm_amd import decoding, ops, synthetic
    from interactvlm_amd import model as M

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = {"7b": synthetic.config_7b, "13b": synthetic.config_13b, "tiny": synthetic.config_tiny}[a.model]()
    weights = synthetic.device_weights(cfg, dev, seed=0)
    vid, bary = synthetic.body_lift_tables(dev)
    model = M.InteractVLMForCausalLM(cfg, weights, dev, lift_tables=(vid, bary))
    del weights
    llm = model.llm
    ids, forced = synthetic.prompt_ids(cfg, n_answer=a.tokens)
    ic, _ = synthetic.images(cfg, dev)
    sync = torch.cuda.synchronize
    ev = lambda: torch.cuda.Event(enable_timing=True)
    H, D = cfg.llama.heads, cfg.llama.hidden // cfg.llama.heads

    def prompts_for(K):
        out = []
        for b in range(K):
            p = ids[0].clone()
            p[-10:] = (p[-10:] + 13 * b) % 31000 + 3  # the last 10 ids differ from question to question
            out.append(p)
        return out

    def wall_ms(fn):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t) * 1e3

    def gpu_ms(fn, reps):
        fn()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    res = {"model": a.model, "tokens": a.tokens, "pairs": a.pairs, "graphs": bool(model.graph_decode), "precision": model.precision,
           "per_K": {}}
    for K in [int(k) for k in a.ks.split(",")]:
        prompts = prompts_for(K)
        P = decoding.shared_prefix_len([p.tolist() for p in prompts], True, model.precision, model.fp8)
        T0 = prompts[0].numel() - 1 + 256
        r = {"prefix_positions": P, "prompt_positions": T0, "prefill_rows": {"plain": K * T0, "shared": P + K * (T0 - P)}}
        gen = lambda share: model.generate_batch(ic, prompts, forced_new_tokens=forced, share_prefix=share)
        o0, o1 = gen(False), gen(True)  # warm-up pair (captures both graphs) + the results side by side
        r["ids_equal"] = all(torch.equal(x[0], y[0]) for x, y in zip(o0, o1))
        r["max_abs_dhidden"] = max(float((x[1] - y[1]).abs().max()) for x, y in zip(o0, o1))
        t = {False: [], True: []}
        for _ in range(a.pairs):
            for share in (False, True):
                t[share].append(wall_ms(lambda: gen(share)))
        r["generate_batch_ms"] = {"plain": _stat(t[False]), "shared": _stat(t[True])}
        gap = r["generate_batch_ms"]["plain"]["median"] - r["generate_batch_ms"]["shared"]["median"]
        r["shared_faster_by_ms"] = round(gap, 4)
        r["beyond_larger_spread"] = bool(gap > max(r["generate_batch_ms"]["plain"]["spread"], r["generate_batch_ms"]["shared"]["spread"]))
        # ---- the pieces -------------------------------------------------------------------------------------------------------
        feats = model.encode_images(ic)
        xs = [model._input_embeds(p, feats[0]) for p in prompts]
        kc, vc = llm.batch_cache(K)
        pre = {False: [], True: []}
        for _ in range(a.pairs):
            pre[False].append(gpu_ms(lambda: llm.forward_packed(xs, kc, vc), 1))
            pre[True].append(gpu_ms(lambda: llm.forward_shared_prefix(xs, P, kc, vc), 1))

        def copy_rows():
            for c in (kc, vc):
                c[:, 1:, :P].copy_(c[:, :1, :P])
        r["prefill_ms"] = {"plain": _stat(pre[False]), "shared": _stat(pre[True]), "prefix_copy_alone": round(gpu_ms(copy_rows, 5), 4),
                           "prefix_copy_mb": round(2 * llm.cfg.layers * (K - 1) * P * H * D * 2 / 1e6, 1)}
        # (the caches now hold the K prompts, every slab complete: both steps and both attention kernels run on this state)
        pos = torch.full((K,), T0 + a.tokens // 2, dtype=torch.int32, device=dev)
        step = {}
        for name, pf in (("plain", None), ("shared", P)):
            st = llm.decode_graph_batch(K, pos, pf)

            def replay():
                st["pos"].copy_(pos)
                st["graph"].replay()
            step[name] = [gpu_ms(replay, 20) for _ in range(a.pairs)]
        r["decode_step_ms"] = {k: _stat(v) for k, v in step.items()}
        qkv = torch.randn(K, 3 * H * D, device=dev)
        pdev = torch.tensor([P], dtype=torch.int32, device=dev)
        scratch = ops.decode_attn_prefix_scratch(K, H, D, dev)
        th, sc = cfg.llama.theta, D ** -0.5
        kinds = {"plain": lambda: ops.llama_decode_attn_batch(qkv, kc[0], vc[0], H, D, pos, th, sc, table=llm.rope),
                 "shared": lambda: ops.llama_decode_attn_batch_prefix(qkv, kc[0], vc[0], H, D, pos, pdev, th, sc, table=llm.rope,
                                                                      scratch=scratch)}
        for f in kinds.values():
            f()
        ops.TIMER.start()
        for _ in range(20):
            for name, f in kinds.items():
                ops.TIMER.time("attn_" + name, 0, f)
        ops.TIMER.stop()
        summ = ops.TIMER.summary()
        r["decode_attention_us_per_layer"] = {name: round(summ["attn_" + name]["avg_us"], 2) for name in kinds}
        r["decode_attention_us_per_layer"]["positions"] = int(pos[0])
        res["per_K"][str(K)] = r
        print(json.dumps({"K": K, **r}), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
