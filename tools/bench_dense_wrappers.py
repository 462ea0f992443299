"""Host cost of the dense wrappers of interactvlm_amd/ops.py: what a change of the Python between the model and the C ABI can move.

    python tools/bench_dense_wrappers.py [--out FILE]                        one run: a JSON line of figures
    python tools/bench_dense_wrappers.py --verdict P0 T0 P1 T1 [--out FILE]  four runs (parent, this, parent, this) -> verdicts

Per-call figures (us): the wall time of N back-to-back calls with one synchronisation at the end, divided by N, at the small shapes of
tests/_dense_bits.py (the kernels take a few microseconds there, so the figure is the host's enqueue cost unless the device is
slower); the median of five such rounds.  sam_forward_ms / prefill_ms: the wall time of one eager ``SamImageEncoder._forward`` (about
320 launches) and of one LLaMA prefill of the synthetic model of tools/bench_stages.py, enqueue to synchronisation; the median of five.

The rule of --verdict is that of profiles/lift_refactor_bench.json: a figure passes if both of this commit's values lie within the
range of the parent's two runs, widened by that range's own width.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_CALLS, ROUNDS = 2000, 5


def per_call_us(fn):
    import torch

    for _ in range(50):
        fn()
    rounds = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N_CALLS):
            fn()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / N_CALLS * 1e6)
    return statistics.median(rounds)


def once_ms(fn):
    import torch

    fn()
    rounds = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(rounds)


def measure():
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import ops, synth, synthetic

    dev = torch.device("cuda:0")
    bf, f32 = torch.bfloat16, torch.float32
    t = lambda key, shape, dtype=bf: torch.from_numpy(synth.synth_normal("bench_dense/" + key, shape, 1.0)).to(dev).to(dtype)
    x, w, b, r = t("x", (48, 128)), t("w", (128, 128)), t("b", (128,)), t("r", (48, 128))
    x1, w1 = t("x1", (1, 256), f32), t("w1", (256, 256))
    xn, g, be = t("xn", (5, 256), f32), t("g", (256,)), t("be", (256,))
    src, idx = t("src", (9, 64), f32), torch.tensor([4, -1, 8, 0, 4, 2, 7], dtype=torch.int32, device=dev)
    q, k, v = (t(n, (2, 70, 4, 64)).permute(0, 2, 1, 3) for n in "qkv")
    H, D, Tmax = 3, 128, 1024
    qkv, kc, vc = t("qkv", (1, 3 * H * D), f32), t("kc", (Tmax, H, D)), t("vc", (Tmax, H, D))
    tab = ops.rope_table(Tmax, D, 10000.0, dev)
    out = {
        "linear_tile_us": per_call_us(lambda: ops.linear(x, w, b, act="gelu", residual=r)),
        "linear_m1_us": per_call_us(lambda: ops.linear(x1, w1, out_f32=True)),
        "layernorm_us": per_call_us(lambda: ops.layernorm(xn, g, be)),
        "gather_rows_us": per_call_us(lambda: ops.gather_rows(src, idx)),
        "attention_us": per_call_us(lambda: ops.attention(q, k, v, 0.125)),
        "decode_attn_us": per_call_us(lambda: ops.llama_decode_attn(qkv, kc, vc, H, D, 385, 10000.0, D ** -0.5, table=tab)),
    }
    cfg = synthetic.config_7b()
    wts = synthetic.device_weights(cfg, dev, seed=0)
    m = M.InteractVLMForCausalLM(cfg, wts, dev, lift_tables=synthetic.body_lift_tables(dev))
    del wts
    ids, _ = synthetic.prompt_ids(cfg)
    _, im = synthetic.images(cfg, dev)
    enc = m.model.visual_model.image_encoder
    out["sam_forward_ms"] = once_ms(lambda: enc._forward(im[0]))
    emb = m.llm.embed_ids(ids[0].to(dev, torch.int32))
    out["prefill_ms"] = once_ms(lambda: m.llm.forward(emb, 0))
    return out


def verdicts(parent, this):
    out = {}
    for key in parent[0]:
        lo, hi = min(p[key] for p in parent), max(p[key] for p in parent)
        allowed = (lo - (hi - lo), hi + (hi - lo))
        vals = [t[key] for t in this]
        slow, fast = [v > allowed[1] for v in vals], [v < allowed[0] for v in vals]
        if not any(slow) and not any(fast):
            verdict = "pass"
        elif any(slow) and any(fast):
            verdict = "fail: both sides"
        else:
            verdict = "fail: " + ("" if all(slow) or all(fast) else "one run ") + ("slower" if any(slow) else "faster")
        out[key] = {"parent": [round(p[key], 3) for p in parent], "this": [round(v, 3) for v in vals],
                    "allowed": [round(a, 3) for a in allowed], "verdict": verdict}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verdict", nargs=4, metavar=("P0", "T0", "P1", "T1"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.verdict:
        runs = [json.load(open(f)) for f in a.verdict]
        res = {"tool": "tools/bench_dense_wrappers.py, one MI355X, one session, in the order parent, this, parent, this",
               "rule": "a figure passes if both of this commit's values lie within the range of the parent's two runs widened by "
                       "that range's own width",
               "verdicts": verdicts(runs[0::2], runs[1::2]),
               "runs": [{"tree": "parent" if i % 2 == 0 else "this", "order": i, "result": r} for i, r in enumerate(runs)]}
    else:
        res = measure()
    text = json.dumps(res, indent=1 if a.verdict else None)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
