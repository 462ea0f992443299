"""Contact-weighted human-object distance: the term of the reference's joint fitting stage that consumes both contact vectors
(optim/optimizer.py ``contact_loss``), as one fused HIP forward + backward (csrc/contact_pair.hip).

    d_ij = |o_i - h_j|,  S = (sum p)(sum q),  L = sum_ij p_i q_j d_ij / S

No [N_o, N_h] array exists anywhere; vertices of probability 0 cost nothing and change no bit of the result.  The rest of
the fit: ``contact_icp`` (the start), ``silhouette`` (mask and centroid terms), ``fit`` (the loop).  There is no CPU fallback.
"""
from __future__ import annotations

import functools

import torch

from . import _lib
from ._args import ValueWithGradients, batch_size, check_devices, check_points, check_vector, side
from ._lib import check

# The longest serial fp32 accumulation of the kernel (IVLM_CONTACT_PAIR_CHAIN of include/ivlm_hip.h: the vertices of one LDS
# tile); what follows it is summed in fp64.  Tests derive their tolerance from it: (L_CHAIN + 8) * 2^-24 * sum |terms|.
L_CHAIN = _lib.header_constant("IVLM_CONTACT_PAIR_CHAIN")

IVLM_F32, IVLM_BF16 = _lib.header_constant("IVLM_F32"), _lib.header_constant("IVLM_BF16")


def validate(obj_verts, human_verts, obj_probs, human_probs):
    """-> (B, batched): raises before anything touches the library"""
    check_points(obj_verts, "obj_verts")
    check_points(human_verts, "human_verts")
    check_vector(obj_probs, obj_verts.shape[-2], "obj_probs", (torch.float32, torch.bfloat16))
    check_vector(human_probs, human_verts.shape[-2], "human_probs", (torch.float32, torch.bfloat16))
    named = [(obj_verts, "obj_verts", 2), (human_verts, "human_verts", 2)]
    B = batch_size(named)
    check_devices(named + [(obj_probs, "obj_probs", 1), (human_probs, "human_probs", 1)])
    return B, obj_verts.dim() == 3 or human_verts.dim() == 3


def one_dtype(p, q):
    """The C ABI takes one p_dtype for both probability vectors: a mixed pair goes in as fp32 (exact: bf16 is a subset).
    -> (p, q contiguous in one dtype, its IVLM_F32 / IVLM_BF16)"""
    if p.dtype != q.dtype:
        p, q = p.float(), q.float()
    return p.contiguous(), q.contiguous(), IVLM_BF16 if p.dtype == torch.bfloat16 else IVLM_F32


def _launch(p, q, obj_verts, human_verts, need):
    """-> (L [B], dL/do [B,No,3] | None, dL/dh [B,Nh,3] | None), the gradients per pose"""
    lib = _lib.load()
    (o, o_bs), (h, h_bs) = side(obj_verts, 2), side(human_verts, 2)
    B = max(o.shape[0], h.shape[0])
    n_o, n_h = o.shape[1], h.shape[1]
    p, q, p_dtype = one_dtype(p, q)
    dev = o.device
    with torch.cuda.device(dev):
        ws, nbytes = _lib.workspace(lib.ivlm_contact_pair_workspace_bytes, "contact_distance", dev, B=B, N_o=n_o, N_h=n_h)
        value = torch.empty(B, dtype=torch.float32, device=dev)
        go = torch.empty(B, n_o, 3, dtype=torch.float32, device=dev) if need[0] else None
        gh = torch.empty(B, n_h, 3, dtype=torch.float32, device=dev) if need[1] else None
        check(lib.ivlm_contact_pair(o.data_ptr(), h.data_ptr(), p.data_ptr(), q.data_ptr(), p_dtype, B, n_o, n_h, o_bs, h_bs,
                                    value.data_ptr(), _lib.ptr(go), _lib.ptr(gh), ws.data_ptr(), nbytes, _lib.stream()), "contact_pair")
    return value, go, gh


def contact_distance(obj_verts, human_verts, obj_probs, human_probs):
    """Contact-probability-weighted mean distance between every object vertex and every human vertex.

    obj_verts [N_o,3] or [B,N_o,3], human_verts [N_h,3] or [B,N_h,3] (fp32, GPU; an unbatched side, or one of batch size 1, is
    shared by the batch of the other), obj_probs [N_o], human_probs [N_h] >= 0 (fp32 or bf16, shared by the batch; constants: no
    gradient flows to them) -> L, shape [] when both sides are unbatched, else [B].  The kernel reads both probability vectors
    in one dtype: of a mixed pair the bf16 vector is upcast to fp32 first, which is exact and costs one small torch kernel.
    Differentiable in both vertex tensors, once: the forward pass computes dL/d(vertices) in the same launch for the sides that
    require grad and saves them as constants, so a double backward (create_graph=True) raises.  The same bits every call."""
    _, batched = validate(obj_verts, human_verts, obj_probs, human_probs)
    value = ValueWithGradients.apply(functools.partial(_launch, obj_probs.detach(), human_probs.detach()), obj_verts, human_verts)
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
