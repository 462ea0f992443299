"""Host side of ``evaluate(exact_sets=...)``: certify the vertex-id sets of a call, or say that it was re-run.

The sets ``{p >= 0.5}`` / ``{p > 0.3}`` of a pass whose per-vertex error is below ``margin`` can differ from the fp32 oracle's
only at vertices within ``margin`` of a threshold (and, through the thresholded object-mesh lift, at pixels whose
sigmoid(logit) is within ``mask_margin`` of the lift's 0.3).  The census kernels (``ops.contact_band_census``,
``ops.mask_band_census``) count both populations on the device; this module lays their outputs out for ONE host read together
with the non-finite flag, decides which images of a call have to be re-run in the ``parity`` mode, cuts those images out of
the arguments of an ``evaluate_batch`` call, and writes the ``result["exact_sets"]`` report.  Nothing here touches the device
except through the ``ops`` functions it is handed, so the bookkeeping is testable without one.
"""
from __future__ import annotations

import torch

DEFAULTS = dict(thresholds=(0.5, 0.3), margin=1e-3, mask_margin=None)
# the parity mode's own distance class to the fp32 oracle (8e-6): the band of the re-run's census
PARITY_MARGIN = 1e-5


def config(exact_sets):
    """None -> None (option off); True -> DEFAULTS; a dict overrides them.  mask_margin None = margin."""
    if exact_sets is None or exact_sets is False:
        return None
    cfg = dict(DEFAULTS)
    if exact_sets is not True:
        unknown = set(exact_sets) - set(cfg)
        if unknown:
            raise ValueError(f"exact_sets: unknown keys {sorted(unknown)} (known: {sorted(cfg)})")
        cfg.update(exact_sets)
    cfg["thresholds"] = tuple(float(t) for t in cfg["thresholds"])
    if not 1 <= len(cfg["thresholds"]) <= 4:
        raise ValueError("exact_sets: 1 to 4 thresholds")
    cfg["margin"] = float(cfg["margin"])
    cfg["mask_margin"] = cfg["margin"] if cfg["mask_margin"] is None else float(cfg["mask_margin"])
    if not (cfg["margin"] >= 0.0 and cfg["mask_margin"] >= 0.0):
        raise ValueError("exact_sets: margins must be >= 0")
    return cfg


def _row_of_base(pc):
    """(base, row) when pc is row `row` of a contiguous fp32 [n, Nv] tensor (the batched body lift returns such views)."""
    base = getattr(pc, "_base", None)
    if (base is None or pc.dtype != torch.float32 or base.dtype != torch.float32 or base.dim() != 2 or pc.dim() != 2
            or pc.shape[0] != 1 or base.shape[1] != pc.shape[1] or not base.is_contiguous() or not pc.is_contiguous()):
        return None, 0
    off = pc.storage_offset() - base.storage_offset()
    if off < 0 or off % pc.shape[1] or off // pc.shape[1] >= base.shape[0]:
        return None, 0
    return base, off // pc.shape[1]


def launch(outs, lifts, thresholds, margin, mask_margin, mask_threshold, ops):
    """Enqueue the census of every result of a call.  lifts: {image index: ("plan", LiftPlan, logits) | ("dense", None, None)}
    for the images that went through the thresholded object-mesh lift.  Contact maps that are rows of ONE [n, Nv] buffer (the
    batched body lift) are censused by one launch with B = n.  -> (parts, layout): int32 device vectors to concatenate for
    the host read, and per image None (no contacts) or (J, mask, rows) with mask in (None, "census", "uncensused")."""
    parts, layout = [], []
    J = len(thresholds)
    shared = {}  # id(base) -> (counts, mindist) of the whole buffer
    for b, o in enumerate(outs):
        pc = o.get("pred_contact_3d")
        if pc is None or pc.numel() == 0:
            layout.append(None)
            continue
        pc = pc.reshape(-1, pc.shape[-1])
        base, row = _row_of_base(pc)
        if base is not None:
            if id(base) not in shared:
                shared[id(base)] = ops.contact_band_census(base, thresholds, margin)
            counts, mind = (t[row: row + 1] for t in shared[id(base)])
        else:
            counts, mind = ops.contact_band_census(pc if pc.dtype == torch.float32 else pc.float(), thresholds, margin)
        parts += [counts.reshape(-1), mind.reshape(-1).view(torch.int32)]
        mask = None
        lift = lifts.get(b)
        if lift is not None:
            if lift[0] == "plan":
                parts.append(ops.mask_band_census(lift[2], lift[1], mask_threshold, mask_margin).reshape(-1))
                mask = "census"
            else:
                mask = "uncensused"
        layout.append((J, mask, int(pc.shape[0])))
    return parts, layout


def read(flags, parts, layout):
    """THE host read of the call: the guard's finite flags (device booleans, may be empty) and the census vectors in one
    device-to-host copy.  -> (finite flag, per image None or {"in_band", "nonfinite", "min_distance", "mask_band",
    "mask_nonfinite"})."""
    head = torch.stack(flags).all().to(torch.int32).reshape(1) if flags else None
    vecs = ([head] if head is not None else []) + list(parts)
    if not vecs:
        return True, [None] * len(layout)
    host = torch.cat(vecs).cpu()
    k = 0
    ok = True
    if head is not None:
        ok = bool(host[0])
        k = 1
    recs = []
    for lay in layout:
        if lay is None:
            recs.append(None)
            continue
        J, mask, rows = lay
        c = host[k: k + rows * (J + 1)].view(rows, J + 1)
        k += rows * (J + 1)
        d = host[k: k + rows * J].view(torch.float32).view(rows, J)
        k += rows * J
        rec = {"in_band": [int(x) for x in c[:, :J].sum(0)], "nonfinite": int(c[:, J].sum()),
               "min_distance": [float(x) for x in d.min(0).values], "mask_band": None, "mask_nonfinite": 0}
        if mask == "census":
            rec["mask_band"], rec["mask_nonfinite"] = int(host[k]), int(host[k + 1])
            k += 2
        elif mask == "uncensused":
            rec["mask_band"] = "uncensused"
        recs.append(rec)
    assert k == host.numel()
    return ok, recs


def undecided(rec):
    """Why the census cannot vouch for this image's sets (None: it can)."""
    if rec is None:
        return None
    if rec["nonfinite"] or rec["mask_nonfinite"]:
        return "nonfinite"
    if rec["mask_band"] == "uncensused":
        return "uncensused"
    if any(rec["in_band"]):
        return "band"
    if rec["mask_band"]:
        return "mask_band"
    return None


def select(ok, recs):
    """-> {image index: reason} of the images to re-run (a failed finite flag is per call: every image)."""
    out = {}
    for b, rec in enumerate(recs):
        why = undecided(rec)
        if not ok and why is None:
            why = "nonfinite"
        if why is not None:
            out[b] = why
    return out


def _census_fields(rec, J):
    if rec is None:  # no mask was decoded: there are no sets
        return {"in_band": [0] * J, "min_distance": [float("inf")] * J, "mask_band": None}
    return {"in_band": list(rec["in_band"]), "min_distance": list(rec["min_distance"]), "mask_band": rec["mask_band"]}


def report(rec, margin, J, parity_rec=None, reason=None):
    """result["exact_sets"] of one image.  Not re-run: certified = the band of the pass is empty.  Re-run: the first pass's
    census, plus the parity pass's own census at PARITY_MARGIN under "parity"; certified = THAT band is empty (False in the rare
    case that even the parity mode sits within its own error of a threshold)."""
    out = {"certified": undecided(rec) is None, "escalated": False, "margin": margin}
    out.update(_census_fields(rec, J))
    if reason is not None:
        out["escalated"] = True
        out["reason"] = reason
        out["parity"] = dict(_census_fields(parity_rec, J), margin=PARITY_MARGIN)
        out["certified"] = undecided(parity_rec) is None
    return out


def _pick(x, idx, B):
    if isinstance(x, torch.Tensor):
        return x[idx] if x.shape[0] == B else x
    if isinstance(x, (list, tuple)) and len(x) == B:
        return [x[i] for i in idx]
    return x


def subset_batch_args(args, idx):
    """The positional arguments of evaluate_batch (images_clip, images, input_ids_list, cam_params, resize_list,
    original_size_list, contact_type, max_new_tokens, forced_new_tokens, eos_token_id, lift2d_dict_path, image_embeddings)
    restricted to the images ``idx``.  Shared entries stay shared: one picture for all prompts (images_clip [1,...]), one
    contact type / forced answer / table path / embedding tensor for all images."""
    (images_clip, images, input_ids_list, cam_params, resize_list, original_size_list, contact_type, max_new_tokens,
     forced_new_tokens, eos_token_id, lift2d_dict_path, image_embeddings) = args
    B = len(input_ids_list)
    idx = list(idx)
    forced = forced_new_tokens
    if forced is not None and len(forced) > 0 and isinstance(forced[0], (list, tuple)):
        forced = [forced[i] for i in idx]
    embs = image_embeddings
    if isinstance(embs, (list, tuple)):
        embs = [embs[i] for i in idx]
    return (_pick(images_clip, idx, B), None if images is None else _pick(images, idx, B), [input_ids_list[i] for i in idx],
            [cam_params[i] for i in idx], [resize_list[i] for i in idx], [original_size_list[i] for i in idx],
            contact_type if isinstance(contact_type, str) else [contact_type[i] for i in idx], max_new_tokens, forced,
            eos_token_id, [lift2d_dict_path[i] for i in idx] if isinstance(lift2d_dict_path, (list, tuple)) else lift2d_dict_path,
            embs)


def splice(outs, idx, sub):
    """outs with the images ``idx`` replaced by the re-run's results ``sub`` (same order)."""
    outs = list(outs)
    for i, o in zip(idx, sub):
        outs[i] = o
    return outs
