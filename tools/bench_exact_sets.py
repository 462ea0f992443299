"""Numbers of evaluate(exact_sets=...): one JSON line.

    python tools/bench_exact_sets.py --model 7b [--images 64] [--reps 20]

  rerun_rate          share of the seeded dp images (bench.py's: seeds 1000 + i) whose default-mode contacts have a vertex within
                      1e-3 of 0.5 / 0.3 - counted with the census kernel on plain evaluate() results, no re-run
  ms_off / ms_certified   evaluate() without the option against evaluate(exact_sets=dict(margin=0.0)) - the certified path: census +
                      the one host read, never a re-run - in ALTERNATING calls on the same model, medians
  ms_escalated        evaluate(exact_sets=dict(margin=1.0)): default pass + census + parity re-run + its census (after one warm call,
                      which rebuilds the bf16 matrices)
  census_us           the contact census launch alone on a [1, Nv] map (event-timed over 200 launches)
  mask_sigmoid_diff   max |sigmoid(logit_default) - sigmoid(logit_parity)| of one call: over all pixels, and over the pixels of the
                      lift tables (what mask_margin is to bound)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import ops, synthetic
    from interactvlm_amd import weights as Wt

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "tiny", "fulldepth"])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    if args.model == "fulldepth":  # the configuration of tests/test_parity_mode_gpu.py::test_full_depth_end_to_end_vs_oracle
        cfg = Wt.IvlmCfg(llama=Wt.LlamaCfg(hidden=1024, layers=32, heads=8, inter=2752, vocab=32003),
                         clip=Wt.ClipCfg(hidden=256, layers=24, heads=4, inter=512), sam=Wt.SamEncCfg())
    else:
        cfg = {"7b": synthetic.config_7b, "tiny": synthetic.config_tiny}[args.model]()
    w = synthetic.device_weights(cfg, dev, seed=0 if args.model != "fulldepth" else 3)
    vid, bary = synthetic.body_lift_tables(dev)
    m = M.InteractVLMForCausalLM(cfg, w, dev, lift_tables=(vid, bary))
    del w
    ids, forced = synthetic.prompt_ids(cfg)
    cams = synthetic.human_cam_params()
    S = cfg.sam.img_size
    sizes = [(S, S)]

    def call(ic, im, **kw):
        out = m.evaluate(ic, im, ids, cams, sizes, sizes, contact_type="hcontact", forced_new_tokens=forced, **kw)
        torch.cuda.synchronize()
        return out

    res = {"model": args.model, "images": args.images}
    ic0, im0 = synthetic.images(cfg, dev, seed=0)
    call(ic0, im0)
    call(ic0, im0, exact_sets=dict(margin=0.0))

    # re-run rate
    flagged, in_band = 0, []
    for i in range(args.images):
        ic, im = synthetic.images(cfg, dev, seed=1000 + i)
        p = call(ic, im)["pred_contact_3d"].float()
        c, _ = ops.contact_band_census(p, (0.5, 0.3), 1e-3)
        c = c.cpu()[0].tolist()
        in_band.append(c)
        flagged += any(c)
    res["rerun_rate"] = flagged / max(args.images, 1)
    res["in_band_mean"] = [sum(c[j] for c in in_band) / max(len(in_band), 1) for j in range(2)]

    # certified call against the plain call, alternating
    off, cert = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        call(ic0, im0)
        off.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        o = call(ic0, im0, exact_sets=dict(margin=0.0))
        cert.append((time.perf_counter() - t) * 1e3)
        assert not o["exact_sets"]["escalated"]
    res["ms_off"], res["ms_certified"] = statistics.median(off), statistics.median(cert)
    res["certified_over_off_pct"] = 100.0 * (res["ms_certified"] / res["ms_off"] - 1.0)

    # the census launch alone
    p = call(ic0, im0)["pred_contact_3d"].float()
    thr = ops.band_thresholds((0.5, 0.3), dev)
    for _ in range(10):
        ops.contact_band_census(p, thr, 1e-3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        ops.contact_band_census(p, thr, 1e-3)
    b.record()
    torch.cuda.synchronize()
    res["census_us"] = a.elapsed_time(b) * 1e3 / 200

    # escalated call, and the masks of the two modes
    d = call(ic0, im0)["pred_masks"][0].float()
    o = call(ic0, im0, exact_sets=dict(margin=1.0))  # warm: rebuilds the bf16 matrices
    assert o["exact_sets"]["escalated"]
    q = o["pred_masks"][0].float()
    diff = (torch.sigmoid(d) - torch.sigmoid(q)).abs()
    res["mask_sigmoid_diff"] = {"all_pixels": float(diff.max()), "table_pixels": float(diff[vid[..., 0] >= 0].max()),
                                "contacts_default_vs_parity": float((call(ic0, im0)["pred_contact_3d"].float()
                                                                     - o["pred_contact_3d"].float()).abs().max())}
    esc = []
    for _ in range(max(3, args.reps // 4)):
        t = time.perf_counter()
        call(ic0, im0, exact_sets=dict(margin=1.0))
        esc.append((time.perf_counter() - t) * 1e3)
    res["ms_escalated"] = statistics.median(esc)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
