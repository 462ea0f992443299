"""The cases of tests/test_lift_bits_gpu.py and tests/golden/make_golden_lift_bits.py: everything deterministic in the mask-to-vertex
lift family - the plan build (count, scan, fill, sort), the plan gather in its three modes, the fused low-res gather and the mask band
census.  A case is a function of the device that returns a list of tensors; ``record`` turns it into strings that compare equal
exactly when every bit does.  The streaming kernels (``lift_mesh_dense``, ``lift_points``) commit float atomics in no fixed order and
are not here: tests/test_lift_stream_gpu.py holds them to a tolerance.

All inputs are seeded from ``synth``, so they are the same numbers wherever the cases run.
"""
import functools
import hashlib

import numpy as np
import torch

from interactvlm_amd import ops, synth

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def encode(t):
    """a tensor -> the hex of its int32 view (fp32 and int32 values); the sha256 of those bytes when they are more than 64, so that
    the golden file stays small"""
    t = t.detach().cpu().contiguous()
    assert t.dtype in (torch.float32, torch.int32), t.dtype
    raw = t.view(torch.int32).numpy().tobytes()
    return raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


def record(name, dev):
    return [f"{tuple(t.shape)} {encode(t)}" for t in CASES[name](dev)]


def _dev(a, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return t.to(dtype) if dtype is not None else t


def _plan_arrays(plan):
    return [torch.tensor([plan.nnz], dtype=torch.int32), plan.row_ptr, plan.ent_pix[: plan.nnz], plan.ent_w[: plan.nnz]]


def _mesh_plan(dev, *table_args, **table_kw):
    vid, bary = synth.synth_mesh_tables(*table_args, **table_kw)
    return vid, ops.LiftPlan(_dev(vid, dev, torch.int32), _dev(bary, dev), table_args[3])


@functools.lru_cache(maxsize=None)
def scene_a(dev):
    """5 views against the gather's 4 waves per block (the view loop runs twice, the second time with one live wave), 997 vertices
    (not a multiple of 8: the grid's tail blocks return early), logits of standard deviation 8 (about 1 % beyond +-20) with one NaN
    and one +inf planted on pixels that vote -> (plan, logits [2,5,64,64], the voting pixels of view 0 as flat indices)"""
    V, H, W, NV = 5, 64, 64, 997
    vid, plan = _mesh_plan(dev, V, H, W, NV, fg=0.4, seed=3)
    logits = synth.synth_normal("lift_bits/a", (2, V, H, W), 8.0, seed=0)
    assert (np.abs(logits) > 20).any()
    voting = [np.flatnonzero(((vid[v] >= 0) & (vid[v] < NV)).all(-1).reshape(-1)) for v in range(V)]
    logits.reshape(2, V, H * W)[0, 0, voting[0][0]] = np.nan
    logits.reshape(2, V, H * W)[1, 1, voting[1][0]] = np.inf
    return plan, _dev(logits, dev), voting


@case
def mesh_plan_and_lift(dev):
    plan, logits, _ = scene_a(dev)
    out = _plan_arrays(plan)
    out += ops.lift_mesh_plan(logits, plan, 0, 20.0, want_nviews=True)
    out += ops.lift_mesh_plan(logits, plan, 1, 0.3, want_nviews=True)
    return out


@case
def mid_and_long_rows(dev):
    """rows of about 2000 entries (LDS bitonic sort with padding, several 256-entry strides of the gather per row) and rows past
    the 8192-entry LDS limit (the sort's global odd-even fallback)"""
    out = []
    for (V, H, W, NV), seed in (((2, 64, 64, 5), 0), ((2, 256, 256, 5), 1)):
        _, plan = _mesh_plan(dev, V, H, W, NV, fg=0.9, seed=seed, adversarial=False)
        rows = (plan.row_ptr[1:] - plan.row_ptr[:-1]).max().item()
        assert 1024 < rows <= 4096 if H == 64 else rows > 8192, rows
        logits = _dev(synth.synth_normal("lift_bits/b", (1, V, H, W), 2.0, seed=seed), dev)
        out += _plan_arrays(plan) + [ops.lift_mesh_plan(logits, plan, 0, 20.0)]
    return out


@case
def point_plan(dev):
    """the point-major plan and mode 2: 37 points, one view without any point, ids at and above the point count"""
    V, H, W, NP = 4, 64, 64, 37
    pid = synth.synth_point_maps(1, V, H, W, NP, seed=2)[0]
    pid[2] = -1
    pid[0, 3, 5:9], pid[1, 40, 7], pid[3, 63, 63] = NP, NP + 3, 1000
    plan = ops.LiftPlan.from_points(_dev(pid, dev, torch.int32), NP)
    probs = _dev(synth.synth_uniform("lift_bits/c", (2, V, H, W), 0, 1, seed=0), dev)
    return _plan_arrays(plan) + list(ops.lift_points_plan(probs, plan, want_nviews=True))


@case
def fused_lowres_lift(dev):
    """lift_plan_lowres_kernel on a small non-square geometry: 16 x 16 low-res masks, a 64-pixel square, a 64 x 43 valid region,
    47 x 31 output pixels; fp32 and bf16 masks, both modes"""
    V, NV, B, oh, ow = 4, 97, 2, 47, 31
    _, plan = _mesh_plan(dev, V, oh, ow, NV, fg=0.4, seed=4)
    low = _dev(synth.synth_normal("lift_bits/d", (B, V, 16, 16), 6.0, seed=0), dev)
    out = []
    for t in (low, low.to(torch.bfloat16)):
        for mode, param in ((0, 20.0), (1, 0.3)):
            out.append(ops.lift_mesh_plan_lowres(t, plan, (64, 43), (oh, ow), 64, mode=mode, param=param))
    return out


@case
def mask_band_census(dev):
    """the census walk over scene (a)'s plan: the logits of its first image (which hold the NaN) with +inf and -inf planted on two
    more voting pixels"""
    plan, logits, voting = scene_a(dev)
    lg = logits[0].clone()
    lg.view(plan.V, -1)[2, int(voting[2][0])] = float("inf")
    lg.view(plan.V, -1)[4, int(voting[4][1])] = float("-inf")
    return [ops.mask_band_census(lg, plan, threshold=0.3, margin=1e-3)]
