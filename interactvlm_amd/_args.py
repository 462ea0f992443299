"""What the Python side of the object-pose fit family (contact_pair, contact_icp, silhouette, pose, mesh_sdf, fit) shares: the argument
checks, the batch axis and stride of a side, and the autograd Function of a term whose forward launch already computed its gradients.

The order of refusals is part of every caller's contract: shapes and dtypes first (``check_points``, ``check_vector``, ``batch_size``),
then ``check_devices``, all of it before ``_lib.load()``.  Tensors travel as ``named`` = [(tensor, name, unbatched rank)].
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def check_points(v, name, dims=(3,), batch=True):
    """v is a float32 tensor [N,D], or [B,N,D] where ``batch`` allows it, with N >= 1 and D in ``dims``"""
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(v).__name__}")
    if v.dim() not in ((2, 3) if batch else (2,)) or v.shape[-1] not in dims or v.shape[-2] < 1 or v.shape[0] < 1:
        D = dims[0] if len(dims) == 1 else "D"
        forms = f"[N,{D}] or [B,N,{D}]" if batch else f"[N,{D}] (no batch axis)"
        raise ValueError(f"{name}: expected {forms} with N >= 1{'' if len(dims) == 1 else f' and D in {tuple(dims)}'}, got {tuple(v.shape)}")
    if v.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {v.dtype}")


def check_vector(v, n, name, dtypes=(torch.float32,), batch=False):
    """v is a tensor [n] (one element per vertex), or [B,n] where ``batch`` allows it, of a dtype in ``dtypes``"""
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(v).__name__}")
    if v.dim() not in ((1, 2) if batch else (1,)) or v.shape[-1] != n or v.shape[0] < 1:
        raise ValueError(f"{name}: expected [{n}]{f' or [B,{n}]' if batch else ' (one per vertex, shared by the batch)'}, got {tuple(v.shape)}")
    if v.dtype not in dtypes:
        raise ValueError(f"{name}: expected {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {v.dtype}")


def batch_size(named):
    """-> B; raises when the batch sizes do not broadcast"""
    B = 1
    for t, name, rank in named:
        b = t.shape[0] if t.dim() == rank + 1 else 1
        if b != 1 and B != 1 and b != B:
            raise ValueError(f"{name}: batch size {b} does not broadcast with {B}")
        B = max(B, b)
    return B


def check_devices(named):
    """all on a GPU (reported in the order of ``named``), all on one device"""
    _lib.require_gpu(named)
    dev = named[0][0].device
    for t, _, _ in named:
        if t.device != dev:
            raise ValueError(f"all tensors must be on one device, got {sorted({str(t.device) for t, _, _ in named})}")


def side(t, rank):
    """-> (contiguous tensor with a batch axis, elements between poses or 0 for a side shared by the batch)"""
    t = (t if t.dim() == rank + 1 else t.unsqueeze(0)).contiguous()
    return t, (t[0].numel() if t.shape[0] > 1 else 0)


def reduce_to(g, shape):
    """per-pose gradient [B,...] -> the shape of the input it belongs to ([...], [1,...] or [B,...])"""
    if len(shape) == g.dim() - 1:
        return g.sum(0) if g.shape[0] > 1 else g[0]
    if shape[0] == 1 and g.shape[0] > 1:
        return g.sum(0, keepdim=True)
    return g


class ValueWithGradients(torch.autograd.Function):
    """A term whose one launch computes its value per pose and the gradients that are needed: ``launch(*inputs, need)`` -> (value [B],
    then per input the per-pose gradient [B,...] or None), need = which inputs require grad.  The gradients are kept as constants;
    the backward scales each by the incoming [B] gradient and reduces it to its input's shape.  Constants of the term (probabilities,
    a prepared mesh) belong to ``launch`` itself, not to ``inputs``."""

    @staticmethod
    def forward(ctx, launch, *inputs):
        value, *ctx.grads = launch(*inputs, ctx.needs_input_grad[1:])
        ctx.shapes = [tuple(x.shape) for x in inputs]
        return value

    @staticmethod
    @once_differentiable  # the saved gradients are constants: a double backward raises instead of returning wrong second derivatives
    def backward(ctx, grad_value):
        return (None, *(None if g is None else reduce_to(grad_value.reshape(-1, *[1] * (g.dim() - 1)) * g, shape)
                        for g, shape in zip(ctx.grads, ctx.shapes)))
