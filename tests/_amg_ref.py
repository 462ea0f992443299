"""What the automatic-mask-generator tests share: a NumPy / float64 restatement of the point grid, of the census (counts and box on
``_resample_ref.post64``), of the stability score, of box NMS with the tie rule, of the run-length encoding and its inverse, and
the one seeded candidate generator of tests/golden/amg_select.npz (one definition for the golden script and the tests).  No GPU in
this module.  tests/test_amg_cpu.py pins the restatement to the reference's own records."""
from __future__ import annotations

import functools

import numpy as np

import _resample_ref as RR

# ---- the golden's geometry ------------------------------------------------------------------------------------------------------------
SEED = 5
LOW = 64                 # the low-res logits are LOW x LOW
IMG = 256                # the padded input frame
PHOTO = (150, 100)       # (H, W)
INPUT = (256, 171)       # get_preprocess_shape(150, 100, 256)
SIDE = 4                 # points per side
BATCH = 5                # points per batch of the golden run
IOU_THRESH, STABILITY_THRESH, OFFSET, NMS_THRESH, MASK_THRESH = 0.88, 0.95, 1.0, 0.7, 0.0
MARGIN = 1e-3            # the distance the golden script asserts between every decision and its threshold


def grid(n):
    """[n*n, 2] float64 (x, y): (k + 0.5) / n per axis from the definition (cell centres), x fastest"""
    side = (np.arange(n, dtype=np.float64) + 0.5) / n
    return np.array([[x, y] for y in side for x in side], dtype=np.float64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def candidates(seed=SEED):
    """-> (low float32 [P,3,LOW,LOW], iou float32 [P,3]), P = SIDE^2, read-only: per candidate one Gaussian blob amp exp(-r^2 / 2 s^2) -
    amp / 2, amp 400 or (one time in three) 40 - the shallow ones fail the stability filter -, s about 3, 6, 10 for the three tokens,
    centres snapped to a coarse lattice so that duplicates exist; IoUs from {0.95, 0.91, 0.97, 0.80} +- 0.01"""
    rng = np.random.default_rng(seed)
    P = SIDE * SIDE
    y, x = np.mgrid[0:LOW, 0:LOW].astype(np.float64)
    low, iou = np.zeros((P, 3, LOW, LOW)), np.zeros((P, 3))
    for p in range(P):
        gy, gx = divmod(p, SIDE)
        cy = (gy + 0.5) / SIDE * INPUT[0] / IMG * LOW  # the point in the low-res frame (the photo fills INPUT / IMG of the square)
        cx = (gx + 0.5) / SIDE * INPUT[1] / IMG * LOW
        for m in range(3):
            sy = round(cy / 16) * 16 + rng.uniform(-1, 1) * (m == 2)
            sx = round(cx / 12) * 12 + rng.uniform(-1, 1) * (m == 2)
            s = (3.0, 6.0, 10.0)[m] * rng.uniform(0.9, 1.1)
            amp = rng.choice([400.0, 400.0, 40.0])
            low[p, m] = amp * np.exp(-((y - sy) ** 2 + (x - sx) ** 2) / (2 * s * s)) - amp * 0.5
            iou[p, m] = rng.choice([0.95, 0.91, 0.97, 0.80]) + rng.uniform(-0.01, 0.01)
    low, iou = low.astype(np.float32), iou.astype(np.float32)
    low.setflags(write=False), iou.setflags(write=False)
    return low, iou


def golden_points():
    """[P,2] float64: the grid scaled to the golden's photo, (x, y) in its pixels"""
    return grid(SIDE) * np.array([[PHOTO[1], PHOTO[0]]], dtype=np.float64)


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def box_of(mask):
    """bool [H,W] -> (x0, y0, x1, y1) inclusive, (0, 0, 0, 0) for an empty mask"""
    ys, xs = np.nonzero(mask)
    return (0, 0, 0, 0) if len(ys) == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def census_of(values, thresholds, shift=0.0):
    """values [n,H,W] -> int64 [n,8]: #(v > hi + shift), #(v > mid + shift), #(v > lo + shift), the box of {v > mid + shift}, 0.
    shift [n,1,1] or a number: +bound / -bound give the two ends of a candidate's bracket"""
    hi, mid, lo = (np.float64(np.float32(t)) for t in thresholds)  # the thresholds as the fp32 numbers the device compares with
    out = np.zeros((values.shape[0], 8), dtype=np.int64)
    for c, t in enumerate((hi, mid, lo)):
        out[:, c] = (values > t + shift).sum(axis=(1, 2))
    inside = values > mid + shift
    for i in range(values.shape[0]):
        out[i, 3:7] = box_of(inside[i])
    return out


def census64(low, img, ins, orig, thresholds, shift=0.0):
    """low [n,h,w] -> the census of post64(low)"""
    return census_of(RR.post64(low, img, ins, orig), thresholds, shift)


def stability32(c_hi, c_lo):
    """float32 c_hi / float32 c_lo (0 / 0 = NaN): torch's true division of two int32 tensors"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(c_hi).astype(np.float32) / np.asarray(c_lo).astype(np.float32)


# ---- NMS ------------------------------------------------------------------------------------------------------------------------------
def box_iou32(a, b):
    """torchvision's arithmetic in float32, in its order; 0 / 0 = NaN"""
    f = np.float32
    a, b = [f(v) for v in a], [f(v) for v in b]
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    inter = max(f(0), min(a[2], b[2]) - max(a[0], b[0])) * max(f(0), min(a[3], b[3]) - max(a[1], b[1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def nms_ordered(boxes, thr, valid=None, margins=None):
    """boxes [n,4] ALREADY in score order -> keep flags int32 [n]: a row is kept when it is valid and no KEPT row before it has IoU
    > thr with it; an invalid row neither keeps nor suppresses.  margins: a list that receives |IoU - thr| of every pair compared."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = len(b)
    thr = np.float32(thr)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    dead, keep = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    zero = np.float32(0)
    for i in range(n):
        if not ok[i] or dead[i]:
            continue
        keep[i] = 1
        r = b[i + 1:]  # box_iou32 of row i against every later row, the same float32 operations
        inter = np.maximum(zero, np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0])) \
            * np.maximum(zero, np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            v = inter / (area[i] + area[i + 1:] - inter)
            alive = ok[i + 1:] & ~dead[i + 1:]
            if margins is not None:
                margins.extend(np.abs(v[alive & np.isfinite(v)].astype(np.float64) - float(thr)).tolist())
            dead[i + 1:] |= alive & (v > thr)
    return keep


def score_order(scores):
    """descending scores, ties to the lower index (our rule: torchvision leaves ties undefined)"""
    return sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))


def nms(boxes, scores, thr, margins=None):
    """batched_nms for one category -> the kept indices in descending score order (int64)"""
    order = score_order(scores)
    keep = nms_ordered([boxes[i] for i in order], thr, margins=margins)
    return np.array([order[k] for k in range(len(order)) if keep[k]], dtype=np.int64)


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------
def rle_encode(mask):
    """bool [H,W] -> run lengths over the column-major pixels, alternating unset / set, the first run unset (possibly 0)"""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])
    return ([0] if flat[0] else []) + np.diff(edges).tolist()


def rle_decode(counts, size):
    """the inverse: run lengths, (H, W) -> bool [H,W]"""
    H, W = size
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    assert flat.size == H * W
    return flat.reshape(W, H).T


# ---- the whole filter stage -----------------------------------------------------------------------------------------------------------
def select_ref(low, iou, points, img, ins, orig, iou_thresh=IOU_THRESH, stability_thresh=STABILITY_THRESH, offset=OFFSET,
               nms_thresh=NMS_THRESH, mask_thresh=MASK_THRESH, values=None, margins=None):
    """low [P,M,h,w], iou [P,M], points [P,2] -> dict of arrays over the kept candidates in NMS order: index, boxes (XYXY), areas,
    predicted_iou, stability (float32), points, masks (bool [K,H,W]); and n_iou / n_stability, the numbers of candidates that pass the
    first and the first two filters.  values: the post-processed logits [P*M,H,W] when the caller has them (default: post64)."""
    P, M = iou.shape
    low, iou = np.asarray(low).reshape(P * M, *low.shape[-2:]), np.asarray(iou).reshape(-1)
    values = RR.post64(low, img, ins, orig) if values is None else values
    cen = census_of(values, (mask_thresh + offset, mask_thresh, mask_thresh - offset))
    active = iou > np.float32(iou_thresh) if iou_thresh > 0 else np.ones(P * M, dtype=bool)
    stab = stability32(cen[:, 0], cen[:, 2])
    with np.errstate(invalid="ignore"):
        valid = active & (stab >= np.float32(stability_thresh)) if stability_thresh > 0 else active
    idx = np.flatnonzero(valid)
    kept = idx[nms(cen[idx, 3:7], iou[idx], nms_thresh, margins=margins)] if len(idx) else idx
    return dict(index=kept.astype(np.int64), boxes=cen[kept, 3:7], areas=cen[kept, 1], predicted_iou=iou[kept], stability=stab[kept],
                points=np.asarray(points, dtype=np.float64)[kept // M], masks=values[kept] > np.float32(mask_thresh),
                n_iou=int(active.sum()), n_stability=int(valid.sum()), census=cen, valid=valid)


@functools.lru_cache(maxsize=None)
def golden_band():
    """per candidate of ``candidates()``: (census at the upper end of its band, census at the lower end, in_band bool [n]) - in_band:
    some pixel lies within ``_resample_ref.bound`` of one of the three thresholds, so its counts are bracketed, not pinned"""
    low = candidates()[0].reshape(-1, LOW, LOW)
    ref, e = RR.post64(low, IMG, INPUT, PHOTO), RR.bound(low, IMG, INPUT, PHOTO)
    th = (MASK_THRESH + OFFSET, MASK_THRESH, MASK_THRESH - OFFSET)
    few, many = census_of(ref, th, e), census_of(ref, th, -e)
    return few, many, (few[:, :3] != many[:, :3]).any(axis=1)
