"""HIP-graph capture and replay, in one place.

Every hot stage of an image (CLIP tower, SAM encoder, SAM mask-decoder chain, the batch-1 and the batched decode step) is a
few hundred launches of 3-30 us kernels with no host decision inside: captured once and replayed as one HIP graph, the host
issues one launch instead.  Same kernels, same order, same stream: bit-identical to the eager launches.

A captured graph bakes in the device pointer of every weight, cache slab and scratch buffer it read: whoever frees or
replaces such a buffer drops the graphs that read it in the same breath (``Cache.clear``, ``Llama._drop_graphs``).
"""
from __future__ import annotations

import os

import torch

from . import ops

# The default of the per-object switches (``use_graph`` of the towers / decoders, ``graph_decode`` of the model): set in the
# environment, it runs every stage eagerly (rocprofv3 --pmc passes crash on replayed graphs).
ON = not os.environ.get("IVLM_NO_GRAPHS")


def enabled(flag, *tensors):
    """May a graph be used now: the caller's switch, every input on the GPU, no capture in progress, the kernel timer off."""
    return (bool(flag) and all(t.is_cuda for t in tensors) and not torch.cuda.is_current_stream_capturing()
            and not ops.TIMER.enabled)


def capture(body, device):
    """-> (graph, what body() returned while it was captured).  body runs once eagerly first, on a fresh side stream that the
    caller's stream then waits for (first-use attribute calls, window maps, lazy module loads, allocator pools: none of it may
    happen inside the capture).  Every graph gets its own private memory pool and its own split-K counter arrays."""
    cur = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        body()
    cur.wait_stream(side)
    g = torch.cuda.CUDAGraph()
    ops._SPLITK_CNT_CAPTURE = {}
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):  # (an RCCL watchdog thread may be polling events)
            out = body()
    finally:
        ops._SPLITK_CNT_CAPTURE = None
    return g, out


class Cache:
    """The captured graphs of one static-input stage (CLIP tower, SAM encoder, SAM decoder), keyed by what selects its launches
    (shapes, dtypes, precision, fp8).  ``run`` captures on a miss, copies the inputs into the graph's static clones, replays on
    the caller's stream and returns clones of the outputs.  ``clear()`` where the stage's weights are replaced."""

    def __init__(self):
        self._ents = {}

    def __len__(self):
        return len(self._ents)

    def clear(self):
        self._ents.clear()

    def run(self, key, fn, inputs, dtype=None):
        """fn(*inputs) -> a tensor or a tuple of tensors; dtype: the element type of the static inputs (default: the inputs')"""
        ent = self._ents.get(key)
        if ent is None:
            static = [t.to(dtype or t.dtype).contiguous().clone() for t in inputs]
            g, out = capture(lambda: fn(*static), inputs[0].device)
            ent = self._ents[key] = (g, static, out)
        g, static, out = ent
        for s, t in zip(static, inputs):
            s.copy_(t)
        g.replay()
        return tuple(o.clone() for o in out) if isinstance(out, tuple) else out.clone()
