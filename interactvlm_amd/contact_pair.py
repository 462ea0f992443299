"""Contact-weighted human-object distance: the term of the reference's joint fitting stage that consumes both contact vectors
(optim/optimizer.py ``contact_loss``), as one fused HIP forward + backward (csrc/contact_pair.hip).

    d_ij = |o_i - h_j|,  S = (sum p)(sum q),  L = sum_ij p_i q_j d_ij / S

No [N_o, N_h] array exists anywhere; vertices of probability 0 cost nothing and change no bit of the result.  The rest of
the fit: ``contact_icp`` (the start), ``silhouette`` (mask and centroid terms), ``fit`` (the loop).  There is no CPU fallback.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check

# The longest serial fp32 accumulation of the kernel (IVLM_CONTACT_PAIR_CHAIN of include/ivlm_hip.h: the vertices of one LDS
# tile); what follows it is summed in fp64.  Tests derive their tolerance from it: (L_CHAIN + 8) * 2^-24 * sum |terms|.
L_CHAIN = 512

IVLM_F32, IVLM_BF16 = 0, 1


def _check_verts(v, name):
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(v).__name__}")
    if v.dim() not in (2, 3) or v.shape[-1] != 3 or v.shape[-2] < 1 or v.shape[0] < 1:
        raise ValueError(f"{name}: expected [N,3] or [B,N,3] with N >= 1, got {tuple(v.shape)}")
    if v.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32 vertices, got {v.dtype}")


def _check_probs(p, n, name, verts_name):
    if not isinstance(p, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(p).__name__}")
    if p.dim() != 1 or p.shape[0] != n:
        raise ValueError(f"{name}: expected [{n}] (one probability per vertex of {verts_name}, shared by the batch), "
                         f"got {tuple(p.shape)}")
    if p.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{name}: expected float32 or bfloat16 probabilities, got {p.dtype}")


def _validate(obj_verts, human_verts, obj_probs, human_probs):
    """-> (B, batched): raises before anything touches the library"""
    _check_verts(obj_verts, "obj_verts")
    _check_verts(human_verts, "human_verts")
    _check_probs(obj_probs, obj_verts.shape[-2], "obj_probs", "obj_verts")
    _check_probs(human_probs, human_verts.shape[-2], "human_probs", "human_verts")
    bo = obj_verts.shape[0] if obj_verts.dim() == 3 else 1
    bh = human_verts.shape[0] if human_verts.dim() == 3 else 1
    if bo != bh and bo != 1 and bh != 1:
        raise ValueError(f"batch sizes {bo} (obj_verts) and {bh} (human_verts) do not broadcast")
    _lib.require_gpu(((obj_verts, "obj_verts"), (human_verts, "human_verts"), (obj_probs, "obj_probs"), (human_probs, "human_probs")))
    devs = {t.device for t in (obj_verts, human_verts, obj_probs, human_probs)}
    if len(devs) != 1:
        raise ValueError(f"all four tensors must be on one device, got {sorted(str(d) for d in devs)}")
    return max(bo, bh), obj_verts.dim() == 3 or human_verts.dim() == 3


def _launch(o, h, p, q, want_go, want_gh):
    """o [Bo,No,3], h [Bh,Nh,3] contiguous fp32, Bo / Bh in (1, B) -> (L [B], dL/do [B,No,3] | None, dL/dh [B,Nh,3] | None)"""
    lib = _lib.load()
    B = max(o.shape[0], h.shape[0])
    n_o, n_h = o.shape[1], h.shape[1]
    if p.dtype != q.dtype:  # the C ABI takes one p_dtype for both vectors: a mixed pair goes in as fp32 (exact: bf16 is a subset)
        p, q = p.float(), q.float()
    p, q = p.contiguous(), q.contiguous()
    dev = o.device
    with torch.cuda.device(dev):
        ws, nbytes = _lib.workspace(lib.ivlm_contact_pair_workspace_bytes, "contact_distance", dev, B=B, N_o=n_o, N_h=n_h)
        value = torch.empty(B, dtype=torch.float32, device=dev)
        go = torch.empty(B, n_o, 3, dtype=torch.float32, device=dev) if want_go else None
        gh = torch.empty(B, n_h, 3, dtype=torch.float32, device=dev) if want_gh else None
        check(lib.ivlm_contact_pair(o.data_ptr(), h.data_ptr(), p.data_ptr(), q.data_ptr(),
                                    IVLM_BF16 if p.dtype == torch.bfloat16 else IVLM_F32, B, n_o, n_h,
                                    n_o * 3 if o.shape[0] > 1 else 0, n_h * 3 if h.shape[0] > 1 else 0, value.data_ptr(),
                                    _lib.ptr(go), _lib.ptr(gh), ws.data_ptr(), nbytes, _lib.stream()), "contact_pair")
    return value, go, gh


def _reduce_to(g, shape):
    """per-pose gradient [B,N,3] -> the shape of the input it belongs to ([N,3], [1,N,3] or [B,N,3])"""
    if len(shape) == 2:
        return g.sum(0) if g.shape[0] > 1 else g[0]
    if shape[0] == 1 and g.shape[0] > 1:
        return g.sum(0, keepdim=True)
    return g


class _ContactDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj_verts, human_verts, obj_probs, human_probs):
        o = (obj_verts if obj_verts.dim() == 3 else obj_verts.unsqueeze(0)).contiguous()
        h = (human_verts if human_verts.dim() == 3 else human_verts.unsqueeze(0)).contiguous()
        want_go, want_gh = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        value, go, gh = _launch(o, h, obj_probs, human_probs, want_go, want_gh)
        ctx.grads = (go, gh)  # dL/do, dL/dh per pose: backward only scales them
        ctx.shapes = (tuple(obj_verts.shape), tuple(human_verts.shape))
        return value

    @staticmethod
    @once_differentiable  # the saved gradients are constants: a double backward raises instead of returning wrong second derivatives
    def backward(ctx, grad_value):
        gv = grad_value.reshape(-1, 1, 1)
        out = [None, None, None, None]  # the probabilities are constants, as in the reference (buffers)
        for i in range(2):
            if ctx.needs_input_grad[i]:
                out[i] = _reduce_to(gv * ctx.grads[i], ctx.shapes[i])
        return tuple(out)


def contact_distance(obj_verts, human_verts, obj_probs, human_probs):
    """Contact-probability-weighted mean distance between every object vertex and every human vertex.

    obj_verts [N_o,3] or [B,N_o,3], human_verts [N_h,3] or [B,N_h,3] (fp32, GPU; an unbatched side, or one of batch size 1, is
    shared by the batch of the other), obj_probs [N_o], human_probs [N_h] >= 0 (fp32 or bf16, shared by the batch; constants: no
    gradient flows to them) -> L, shape [] when both sides are unbatched, else [B].  The kernel reads both probability vectors
    in one dtype: of a mixed pair the bf16 vector is upcast to fp32 first, which is exact and costs one small torch kernel.
    Differentiable in both vertex tensors, once: the forward pass computes dL/d(vertices) in the same launch for the sides that
    require grad and saves them as constants, so a double backward (create_graph=True) raises.  The same bits every call."""
    _, batched = _validate(obj_verts, human_verts, obj_probs, human_probs)
    value = _ContactDistance.apply(obj_verts, human_verts, obj_probs.detach(), human_probs.detach())
    return value if batched else value[0]


def contact_agreement(out_h, out_o, human_verts, obj_verts):
    """The distance for the two results of a joint ``evaluate`` (contact_type 'hcontact' and 'ocontact'): out_h / out_o are
    the result dicts (or their ``pred_contact_3d`` tensors), human_verts / obj_verts the posed meshes they were predicted on."""
    def probs(out, name):
        pc = out["pred_contact_3d"] if isinstance(out, dict) else out
        if pc is None:
            raise ValueError(f"{name}: the result holds no pred_contact_3d")
        return pc.detach().reshape(-1)

    return contact_distance(obj_verts, human_verts, probs(out_o, "out_o"), probs(out_h, "out_h"))
