"""evaluate / evaluate_batch(exact_sets=...): the band census decides whether the default-mode result stands or the call is re-run
in the parity mode.  Inputs of the toy of tests/test_model_gpu.py (its helper _toy: lift tables, cameras, image generator) on
synthetic.config_tiny(), the small configuration whose fp32 oracle tests/test_parity_mode_gpu.py builds: the toy's own CLIP head
size is one the parity mode's split-operand attention does not take, so a re-run is impossible on it.  One model per module.

Weights: the plain synthetic weights, rounded to bf16 values, identically for the HIP model and the fp32 oracle."""
import math

import numpy as np
import pytest

from test_model_gpu import _toy

pytestmark = pytest.mark.gpu

SIZES = [(1024, 1024)]
KEYS = {"output_ids", "pred_masks", "pred_contact_3d"}


def _gained(w, gain):
    return {k: (v * gain if "output_hypernetworks_mlps" in k and ".layers.2." in k else v) for k, v in w.items()}


def _images(seed, cuda):
    import torch

    from interactvlm_amd import synth

    bf = torch.bfloat16
    ic = torch.from_numpy(synth.synth_normal("mf/images_clip", (1, 3, 224, 224), 1.0, seed)).to(bf)
    im = torch.from_numpy(synth.synth_normal("mf/images", (1, 4, 3, 1024, 1024), 1.0, seed)).to(bf)
    return ic.to(cuda), im.to(cuda)


@pytest.fixture(scope="module")
def toy(hip_lib, cuda, golden_dir):
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt

    torch.set_grad_enabled(False)
    from interactvlm_amd import synthetic

    _, _, _, _, _, cams, tables = _toy(golden_dir)
    cfg = synthetic.config_tiny()
    prompt, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    ids = torch.cat([prompt[0], torch.tensor(forced)])
    w = {k: v.to(torch.bfloat16).float() for k, v in Wt.synth_weights(Wt.ivlm_spec(cfg)).items()}
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    assert m.precision == "default"
    ic, im = _images(0, cuda)
    kw = dict(forced_new_tokens=ids[40:].tolist())
    args = (ic, im, ids[None, :40], cams, SIZES, SIZES)
    base = m.evaluate(*args, **kw)
    return dict(m=m, w=w, cfg=cfg, ids=ids, cams=cams, tables=tables, args=args, kw=kw, base=base)


def _same(a, b):
    import torch

    return (torch.equal(a["output_ids"], b["output_ids"]) and torch.equal(a["pred_contact_3d"], b["pred_contact_3d"])
            and all(torch.equal(x, y) for x, y in zip(a["pred_masks"], b["pred_masks"])))


def _parity(m, fn):
    m.set_precision("parity")
    try:
        return fn()
    finally:
        m.set_precision("default")


def test_option_off_changes_nothing(toy):
    m = toy["m"]
    off = m.evaluate(*toy["args"], exact_sets=None, **toy["kw"])
    assert set(off) == KEYS == set(toy["base"]) and _same(off, toy["base"])
    import torch

    ic, im = torch.cat([toy["args"][0]] * 2), torch.cat([toy["args"][1]] * 2)
    bargs = (ic, im, [toy["ids"][:40]] * 2, [toy["cams"][0]] * 2, SIZES * 2, SIZES * 2)
    plain = m.evaluate_batch(*bargs, forced_new_tokens=toy["ids"][40:].tolist())
    outs = m.evaluate_batch(*bargs, forced_new_tokens=toy["ids"][40:].tolist(), exact_sets=None)
    assert len(outs) == len(plain) == 2
    for a, b in zip(outs, plain):
        assert set(a) == KEYS == set(b) and _same(a, b)


def test_band_forced_empty_returns_the_default_result(toy):
    m = toy["m"]
    before = dict(m.recomputations or {})
    out = m.evaluate(*toy["args"], exact_sets=dict(margin=0.0), **toy["kw"])
    assert _same(out, toy["base"]) and set(out) == KEYS | {"exact_sets"}
    es = out["exact_sets"]
    assert es["certified"] is True and es["escalated"] is False and es["in_band"] == [0, 0] and es["margin"] == 0.0
    assert es["mask_band"] is None and len(es["min_distance"]) == 2 and all(0.0 < d < 1.0 for d in es["min_distance"])
    p = toy["base"]["pred_contact_3d"].float().cpu()
    assert es["min_distance"] == [float((p - t).abs().min()) for t in (0.5, 0.3)]
    assert (m.recomputations or {}) == before and m.precision == "default"  # no mode switch: no parity kernel ran


def test_band_forced_non_empty_returns_the_parity_result(toy):
    m = toy["m"]
    n0 = (m.recomputations or {}).get("parity", 0)
    out = m.evaluate(*toy["args"], exact_sets=dict(margin=1.0), **toy["kw"])
    assert m.precision == "default" and m.llm.precision == "f16" and m.recomputations["parity"] == n0 + 1
    ref = _parity(m, lambda: m.evaluate(*toy["args"], **toy["kw"]))
    assert _same(out, ref) and not _same(out, toy["base"])
    es = out["exact_sets"]
    assert es["escalated"] is True and es["reason"] == "band" and es["in_band"] == [6890, 6890] and es["margin"] == 1.0
    assert es["parity"]["margin"] == 1e-5
    p = ref["pred_contact_3d"].float().cpu()
    assert es["parity"]["in_band"] == [int(((p - t).abs() <= np.float32(1e-5)).sum()) for t in (0.5, 0.3)]
    assert es["certified"] is (sum(es["parity"]["in_band"]) == 0)
    assert _same(m.evaluate(*toy["args"], **toy["kw"]), toy["base"])  # back in the default mode, same bits as before


def test_sets_equal_the_oracles_over_three_seeds(toy):
    """margin = 1e-3 against the fp32 oracle (oracle.pipeline.model_forward on the same bf16-valued weights, as
    test_parity_mode_gpu.test_evaluate_parity_mode_vs_oracle builds it): the returned sets {p >= 0.5} and {p > 0.3} equal the
    oracle's exactly for every seed, and the seeds must show BOTH outcomes - one that the census certifies in the default mode and
    one that it re-runs.
    Route: the plain weights, no hypernetwork gain - the seeds were chosen from the fp32 oracle's own contacts.  Seed 0: every
    contact in [0.359, 0.490], nothing within 9e-3 of a threshold - certified whatever the default mode's 2e-4 does.  Seed 4:
    [0.398, 0.520] with 19 vertices within 1e-3 of 0.5 - re-run.  Seed 1: [0.379, 0.501] with 2 vertices in the band - close to
    the edge, either outcome is legitimate; its sets must equal the oracle's all the same."""
    import torch

    from interactvlm_amd import synth
    from oracle import pipeline as P

    m, cfg, ids, cams = toy["m"], toy["cfg"], toy["ids"], toy["cams"]
    escalated, equal = [], []
    for seed in (0, 1, 4):
        ic, im = _images(seed, m.device)
        ref = P.model_forward(toy["w"], cfg, im[0].float().cpu(), ic.float().cpu(), ids, cams[0], toy["tables"])["pred_contact"]
        out = m.evaluate(ic, im, ids[None, :40], cams, SIZES, SIZES, exact_sets=dict(margin=1e-3), **toy["kw"])
        p, es = out["pred_contact_3d"].float().cpu(), out["exact_sets"]
        flips = [int(((p >= 0.5) != (ref >= 0.5)).sum()), int(((p > 0.3) != (ref > 0.3)).sum())]
        print(f"\n[exact_sets, seed {seed}] escalated {es['escalated']} certified {es['certified']} in_band {es['in_band']} "
              f"min_distance {es['min_distance']} max|dp| vs oracle {float((p - ref).abs().max()):.2e} flips {flips}")
        escalated.append(es["escalated"])
        equal.append(flips == [0, 0])
    assert all(equal)  # every returned result, certified or re-run, has exactly the oracle's sets at both thresholds
    assert escalated[0] is False and escalated[2] is True  # both outcomes, from the default-mode run alone


def test_evaluate_batch_reruns_a_strict_subset(toy):
    """Four images; the margin is put between the rows' reported minimum distances, so that the census flags exactly two of them.
    Flagged rows = the rows of ONE parity evaluate_batch call over that subset (the call the policy makes), unflagged rows = the
    default batch's rows, all bit for bit; one report per image.  Against a parity batch over ALL four images the flagged rows are
    compared approximately only (1e-4, ten times the parity mode's distance class): the batch size selects the skinny-GEMM kernels
    of the decode step, so rows of batches of different sizes need not share their last bits - the policy promises the subset
    call's result, not the full batch's."""
    import torch

    m, ids, cams = toy["m"], toy["ids"], toy["cams"]
    pics = [_images(s, m.device) for s in (0, 1, 2, 3)]
    ic, im = torch.cat([p[0] for p in pics]), torch.cat([p[1] for p in pics])
    prompts, cam_b, sizes = [ids[:40]] * 4, [cams[0]] * 4, SIZES * 4
    kw = dict(forced_new_tokens=ids[40:].tolist())
    base = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, exact_sets=dict(margin=0.0), **kw)
    assert [o["exact_sets"]["escalated"] for o in base] == [False] * 4
    dist = [min(o["exact_sets"]["min_distance"]) for o in base]
    order = sorted(range(4), key=lambda b: dist[b])
    assert dist[order[1]] < dist[order[2]]
    margin = 0.5 * (dist[order[1]] + dist[order[2]])
    flagged = sorted(order[:2])
    n0 = (m.recomputations or {}).get("parity", 0)
    outs = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, exact_sets=dict(margin=margin), **kw)
    assert m.recomputations["parity"] == n0 + 1 and m.precision == "default"  # one re-run call for both images
    assert [o["exact_sets"]["escalated"] for o in outs] == [b in flagged for b in range(4)]
    sub = _parity(m, lambda: m.evaluate_batch(ic[flagged], im[flagged], [prompts[b] for b in flagged], cam_b[:2], sizes[:2],
                                              sizes[:2], **kw))
    full = _parity(m, lambda: m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, **kw))
    for i, b in enumerate(flagged):
        assert _same(outs[b], sub[i])
        print(f"\n[exact_sets batch] image {b}: re-run row vs the row of a parity batch over all four: max |dp| = "
              f"{float((outs[b]['pred_contact_3d'] - full[b]['pred_contact_3d']).abs().max()):.2e}")
        assert float((outs[b]["pred_contact_3d"] - full[b]["pred_contact_3d"]).abs().max()) < 1e-4
        assert outs[b]["exact_sets"]["reason"] == "band" and outs[b]["exact_sets"]["margin"] == margin
    for b in range(4):
        if b not in flagged:
            assert _same(outs[b], base[b]) and outs[b]["exact_sets"]["certified"] is True
            assert outs[b]["exact_sets"]["min_distance"] == base[b]["exact_sets"]["min_distance"]
    # deferred: the finaliser does the census and the re-run
    fin = m.evaluate_batch(ic, im, prompts, cam_b, sizes, sizes, exact_sets=dict(margin=margin), deferred=True, **kw)
    outs2 = fin()
    assert all(_same(a, b) and a["exact_sets"] == b["exact_sets"] for a, b in zip(outs, outs2))


def test_object_mesh_path_censuses_the_plan_pixels(hip_lib, cuda, tmp_path):
    """The thresholded object-mesh lift: a single-use table (dense path, no plan) is "uncensused" and re-run; a plan-backed call
    gets the pixel census at the lift's 0.3 and stands when that band is empty; a logit planted at logit(0.3) on a plan pixel
    forces the re-run.  Weights: hypernetwork gain 1024 (masks saturate: no natural pixel within 1e-6 of 0.3; contacts are 0 or 1)."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import render, synth, synthetic
    from interactvlm_amd import weights as Wt
    from oracle import raster as R

    torch.set_grad_enabled(False)
    v, f = R.icosphere(3)
    vid, bary, nv = render.object_lift_tables(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), "4MV-Z_HM_BM")
    path = str(tmp_path / "lift2d_dict.pkl")
    render.save_lift2d_dict(path, vid, bary, nv)
    cfg = synthetic.config_tiny()
    cfg.oC_loss_weight, cfg.oC_sam_view_type = 1.0, "4MV-Z_HM_BM"
    w = _gained(Wt.synth_weights(Wt.ivlm_spec(cfg)), 1024.0)
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    ids, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=6)
    cams = synthetic.human_cam_params()
    ic, im = synthetic.images(cfg, cuda)
    call = lambda **kw: m.evaluate(ic, im, ids, cams, SIZES, SIZES, forced_new_tokens=forced, contact_type="ocontact",
                                   lift2d_dict_path=path, **kw)
    opt = dict(margin=1e-3, mask_margin=1e-6)
    first = call(exact_sets=opt)  # first sight of the file: the dense kernel streams the tables, nothing to census
    es = first["exact_sets"]
    assert es["mask_band"] == "uncensused" and es["escalated"] is True and es["reason"] == "uncensused"
    assert m.recomputations == {"parity": 1} and m.precision == "default"
    assert isinstance(es["parity"]["mask_band"], int)  # (the re-run was the file's second sight: it built and censused the plan)
    second = call(exact_sets=opt)  # plan-backed now
    es = second["exact_sets"]
    print(f"\n[exact_sets object] plan-backed call: {es}")
    assert es["mask_band"] == 0 and es["in_band"] == [0, 0] and es["escalated"] is False and es["certified"] is True
    assert m.recomputations == {"parity": 1} and second["pred_contact_3d"].shape == (1, nv)
    assert torch.equal(second["pred_contact_3d"], call()["pred_contact_3d"])
    # plant logit(0.3) on a pixel of the plan (a pixel inside a triangle: three entries), in the masks the lift receives
    mesh = m.object_3d_contact_predictor
    vw, y, x = [int(t) for t in (vid[..., 0] >= 0).nonzero()[0]]
    lift = mesh._lift

    def planted(seg_maps, tables_, cache_key=None):
        s = seg_maps[0].clone()
        s[vw, y, x] = math.log(0.3 / 0.7)
        return lift([s], tables_, cache_key=cache_key)

    mesh._lift = planted
    try:
        third = call(exact_sets=opt)
    finally:
        del mesh._lift
    es = third["exact_sets"]
    assert es["escalated"] is True and es["reason"] == "mask_band" and es["mask_band"] == 3 and es["in_band"] == [0, 0]
    assert es["certified"] is False and es["parity"]["mask_band"] == 3  # (the plant sits in the parity pass's masks as well)
    assert m.recomputations == {"parity": 2} and m.precision == "default"


def test_nonfinite_fallback_parity(hip_lib, cuda, golden_dir):
    """The overflow of test_model_gpu.test_nonfinite_result_of_an_fp16_mode_is_recomputed_in_bf16 (gate / up projections scaled by
    2^11: SiLU(gate) * up leaves fp16's range) with nonfinite_fallback="parity": the guard recomputes in the parity mode and says
    so; with exact_sets on, the non-finite first pass is the reason of the re-run."""
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import weights as Wt

    from interactvlm_amd import synthetic

    _, _, _, images_clip, images, cams, tables = _toy(golden_dir)
    cfg = synthetic.config_tiny()  # (see the module docstring)
    prompt, forced = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=8)
    ids = torch.cat([prompt[0], torch.tensor(forced)])
    w = dict(Wt.synth_weights(Wt.ivlm_spec(cfg)))
    bf = torch.bfloat16
    for n in ("gate_proj", "up_proj"):
        k = f"model.layers.0.mlp.{n}.weight"
        w[k] = (w[k].float() * 2048.0).to(bf)
    ic, im = images_clip.to(bf).to(cuda), images.to(bf).to(cuda)
    args = (ic, im, ids[None, :40], cams, SIZES, SIZES)
    kw = dict(forced_new_tokens=ids[40:].tolist())
    assert M.InteractVLMForCausalLM.nonfinite_fallback == "bf16"  # the default is untouched
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables, nonfinite_fallback="parity")
    assert m.precision == "default" and m.nonfinite_guard and m.nonfinite_fallback == "parity"
    with pytest.warns(UserWarning, match="recomputed in the parity mode"):
        out = m.evaluate(*args, **kw)
    assert out.get("recomputed_in_parity") is True and "recomputed_in_bf16" not in out and m.precision == "default"
    assert m.recomputations == {"parity": 1} and bool(torch.isfinite(out["pred_contact_3d"]).all())
    m.set_precision("parity")
    m.llm.decode_packed = False  # (the guard's recomputation decodes on the bf16 weights: fp32 range)
    ref = m.evaluate(*args, **kw)
    assert torch.equal(out["pred_contact_3d"], ref["pred_contact_3d"]) and torch.equal(out["output_ids"], ref["output_ids"])
    m.llm.decode_packed = True
    m.set_precision("default")
    es = m.evaluate(*args, exact_sets=True, **kw)["exact_sets"]
    assert es["escalated"] is True and es["reason"] == "nonfinite"
