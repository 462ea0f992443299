"""The greedy decode loop of ``generate`` / ``generate_batch``, and its speculative variant (``generate(draft=...)``).

One loop decides for B >= 1 sequences what to feed and when to stop (EOS, or each sequence's length cap), with forced ids or
running free; a step object enqueues the decode work of one token per sequence and puts its hidden rows where they belong.
Four kinds share one interface: one sequence or B, a replayed HIP graph (``Llama.decode_graph`` / ``decode_graph_batch``)
or eager launches.  ``step(tok, out=None)`` consumes ids ``tok`` (int32 [B] on the device; the single-sequence steps also take
a host int) and returns the argmax of every row: written into ``out`` when given, else a tensor of its own.
"""
from __future__ import annotations

import torch

from . import ops
from .constants import IMAGE_TOKEN_INDEX

_ring = None

# the model precision modes (InteractVLMForCausalLM.set_precision) whose batched decode can share a prompt prefix: one K / V plane per
# cache ("default": fp16 rows, "bf16"); the "parity" modes keep hi + lo planes and run the plain path, as speculative decoding does
SHARED_PREFIX_MODES = ("default", "bf16")


def shared_prefix_len(prompts, one_picture, mode="default", fp8=False, image_rows=256, image_id=IMAGE_TOKEN_INDEX):
    """The number P of leading SPLICED positions that are identical in all B sequences, or 0 = take the plain batched path.
    prompts: B id lists (the image id stands for its ``image_rows`` feature rows); one_picture: they refer to the same picture
    (``images_clip.shape[0] == 1``), so equal ids mean equal rows.  P <= min(T0) - 1: every sequence keeps at least one prompt row of
    its own (its last prompt row is what lm_head reads).  0 when: B == 1; several pictures (the text before the image alone is not
    worth a second pass); P <= 16 or <= 16 suffix rows in all (both passes are tile GEMMs, M > 16); a mode outside
    SHARED_PREFIX_MODES, or fp8.  Pure host code."""
    prompts = [[int(t) for t in p] for p in prompts]
    B = len(prompts)
    if B < 2 or not one_picture or fp8 or mode not in SHARED_PREFIX_MODES:
        return 0
    n = 0  # common leading ids
    while n < min(len(p) for p in prompts) and all(p[n] == prompts[0][n] for p in prompts):
        n += 1
    spliced = lambda ids: len(ids) + sum(image_rows - 1 for t in ids if t == image_id)
    T0 = [spliced(p) for p in prompts]
    P = min(spliced(prompts[0][:n]), min(T0) - 1)
    if P <= 16 or sum(T0) - B * P <= 16:
        return 0
    return P


def _id_ring(n):
    """pinned host int32 array of >= n generated ids (written by asynchronous device-to-host copies, read one step late)"""
    global _ring
    if _ring is None or _ring.numel() < n:
        _ring = torch.empty(max(n, 64), dtype=torch.int32, pin_memory=torch.cuda.is_available())
    return _ring


class _Step:
    st = None  # the captured step's static buffers (graph kinds)

    def __init__(self, llm, hidden):
        self.llm, self.hidden = llm, hidden

    def event(self):
        """an event behind the work enqueued so far"""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.hidden.device))
        return ev


class SingleGraph(_Step):
    """one sequence, one replay of Llama.decode_graph per token (embed -> layers -> lm_head -> argmax, position read from and
    advanced on the device); hidden [T0 + n_max, H]: the row of position p goes to hidden[p]"""

    def __init__(self, llm, hidden, T0):
        super().__init__(llm, hidden)
        self.st, self.pos = llm.decode_graph(T0), T0

    def __call__(self, tok, out=None):
        st = self.st
        if isinstance(tok, torch.Tensor):
            st["tok"].copy_(tok)
        else:
            st["tok"].fill_(tok)
        st["graph"].replay()
        self.hidden[self.pos: self.pos + 1].copy_(st["hidden"])
        self.pos += 1
        return st["nxt"].clone() if out is None else out.copy_(st["nxt"])

    def resume(self, n, v):
        """continue after a verify pass (state v) that kept n rows: from the position and token of its accept step"""
        self.pos += n
        self.st["pos"].copy_(v["pos"])
        self.st["tok"].copy_(v["tok"])


class SingleEager(_Step):
    """one sequence, the decode step as eager launches (Llama.forward at a host position)"""

    def __init__(self, llm, hidden, T0):
        super().__init__(llm, hidden)
        self.pos = T0

    def __call__(self, tok, out=None):
        llm = self.llm
        if not isinstance(tok, torch.Tensor):
            tok = torch.tensor([tok], dtype=torch.int32, device=self.hidden.device)
        h = llm.forward(llm.embed_ids(tok), self.pos)
        self.hidden[self.pos: self.pos + 1].copy_(h)
        self.pos += 1
        nxt = ops.argmax(llm.logits(h))
        return nxt if out is None else out.copy_(nxt)

    def resume(self, n, v):
        self.pos += n


class BatchGraph(_Step):
    """B sequences, one replay of Llama.decode_graph_batch per token; hidden [B, T, H]: the row of sequence b at position p goes to
    hidden[b, p] (positions read from the device before the replay advances them)"""

    def __init__(self, llm, hidden, pos, prefix=None):
        super().__init__(llm, hidden)
        self.st = llm.decode_graph_batch(pos.numel(), pos, prefix)  # (prefix: the shared prefix length P on the host, or None)
        self.rows = torch.arange(pos.numel(), device=pos.device)

    def __call__(self, tok, out=None):
        st = self.st
        st["tok"].copy_(tok)
        idx = st["pos"].to(torch.int64)  # positions BEFORE the step's += 1
        st["graph"].replay()
        nxt = st["nxt"].clone() if out is None else st["nxt"]
        self.hidden[self.rows, idx] = st["hidden"]
        return nxt if out is None else out.copy_(nxt)


class BatchEager(_Step):
    """B sequences, Llama.decode_step_batch as eager launches on the cache slabs (kc, vc, lo) at device positions pos; prefix: the
    shared prefix length P on the host, or None"""

    def __init__(self, llm, hidden, pos, caches, prefix=None):
        super().__init__(llm, hidden)
        self.pos, self.caches = pos, caches
        self.prefix = None if prefix is None else torch.tensor([int(prefix)], dtype=torch.int32, device=pos.device)
        self.rows = torch.arange(pos.numel(), device=pos.device)

    def __call__(self, tok, out=None):
        llm = self.llm
        # (finished sequences keep stepping - their rows are ignored; a sequence whose position has reached the end of its
        #  cache slab is skipped by the attention kernel: nothing is appended past Tmax)
        h = llm.decode_step_batch(llm.embed_ids(tok.contiguous()), self.pos, *self.caches, prefix=self.prefix)
        idx = self.pos.to(torch.int64)
        nxt = ops.argmax(llm.logits(h))
        self.pos = self.pos + 1
        self.hidden[self.rows, idx] = h
        return nxt if out is None else out.copy_(nxt)


def greedy(step, nxt, n_seq, eos, forced=None):
    """Greedy search of B = len(n_seq) sequences from nxt (int32 [B] on the device: the argmax of each prompt's last row, id 0).
    Sequence b stops after EOS or its n_seq[b]-th id; the others keep stepping until every one has stopped.
    forced = (host ids [B][n_max], device int32 [n_max, B]): feed these instead of the argmax (which is still computed).
    -> (new ids per sequence, the argmax tensors of steps 0 .. len - 1).

    Running free there is no host round trip per token (reference loop: InteractVLM.py:524-531).  The argmax of step s stays on
    the device and is the token of step s + 1; every id is also copied - asynchronously - into a pinned host array.  The host
    keeps ONE step queued ahead of the one it is waiting for: before it enqueues step s + 1 it waits for the event of step s - 1
    and reads id s - 1 from the pinned array - so the GPU never idles between replays, and when the last sequence stops at id k
    exactly one speculative step (the one that consumed id k) has been enqueued: its hidden and KV rows lie beyond the returned
    lengths and are dropped."""
    B, n_max = len(n_seq), max(n_seq)
    new = [[] for _ in range(B)]
    done = [False] * B

    def absorb(toks):  # the ids of one step, in order: append to the sequences still running -> have all stopped?
        for b in range(B):
            if not done[b]:
                new[b].append(int(toks[b]))
                done[b] = toks[b] == eos or len(new[b]) >= n_seq[b]
        return all(done)

    if forced is not None:
        host, dev = forced
        amax = [nxt]
        for s in range(n_max):
            if absorb([f[s] for f in host]):
                break
            amax.append(step(dev[s]))
        return new, amax
    ring = _id_ring(n_max * B)[: n_max * B].view(n_max, B)
    ids = torch.empty(n_max, B, dtype=torch.int32, device=nxt.device)
    ids[0].copy_(nxt)
    ring[0].copy_(nxt, non_blocking=True)
    evs, amax = [step.event()], []

    def read():  # the next id of every sequence, once its copy has landed -> have all stopped?
        s = len(amax)
        evs[s].synchronize()
        amax.append(ids[s])
        return absorb(ring[s].tolist())

    for s in range(n_max - 1):  # step s consumes id s and produces id s + 1: enqueued once id s - 1 is known
        if s >= 1 and read():
            break
        ring[s + 1].copy_(step(ids[s], out=ids[s + 1]), non_blocking=True)
        evs.append(step.event())
    while not all(done):
        read()
    return new, amax


def speculative(step, nxt, n_max, eos, draft):
    """The free-running greedy loop of one sequence with verify passes (generate(draft=...)).  Per round the host knows every id so
    far and asks the drafter for up to 15 ids to follow; with a proposal d1 .. dm the rows [t, d1 .. dm] (t = last id, padded to a
    bucket of VERIFY_BUCKETS) run through ONE Llama.verify_step at positions pos .. pos+m, the accept step finds n_acc (leading d_j
    equal to the argmax of row j-1), and d1 .. d_n_acc + argmax(row n_acc) are emitted, hidden rows 0 .. n_acc kept; the host reads
    n_acc and the next id once per pass.  Without a proposal the plain step runs (a graph step continues from the accept step's
    position and token).  Stops exactly at EOS or n_max (rows past the stop are dropped, as the plain loop drops its one
    speculative step); no row is written past max_len (n_max already keeps every fed position below it).
    -> (new ids, their argmax tensors, statistics)."""
    llm = step.llm
    kmax = max(llm.VERIFY_BUCKETS)
    new_ids, amax = [int(nxt.item())], [nxt]
    stats = dict(passes=0, plain_steps=0, proposed=0, accepted=0, pattern=[])
    observe = getattr(draft, "observe", None)
    while new_ids[-1] != eos and len(new_ids) < n_max:
        rem = n_max - len(new_ids)  # ids still to emit; the fed rows stay below T0 + n_max - 1 <= max_len - 1
        prop = [int(t) for t in draft.propose(list(new_ids), kmax)][: min(kmax - 1, rem - 1)]
        m = len(prop)
        if m == 0:  # the plain step, then one read-back
            stats["plain_steps"] += 1
            amax.append(step(new_ids[-1]))
            new_ids.append(int(amax[-1].item()))
            continue
        kb = next(b for b in llm.VERIFY_BUCKETS if b >= m + 1)
        fed = torch.tensor([new_ids[-1]] + prop + [new_ids[-1]] * (kb - 1 - m), dtype=torch.int32)
        st = llm.verify_graph(kb) if step.st is not None else llm.verify_state(kb)
        st["pos"].fill_(step.pos)
        st["ids"].copy_(fed)
        st["nd"].fill_(m)
        if step.st is not None:
            st["graph"].replay()
        else:
            llm.verify_pass(st)
        n_acc, tok = torch.cat([st["n_acc"], st["tok"]]).tolist()  # (the one read-back of the pass)
        stats["passes"] += 1
        stats["proposed"] += m
        stats["accepted"] += n_acc
        stats["pattern"].append((m, n_acc))
        if observe is not None:
            observe(m, n_acc)
        va = st["amax"][: n_acc + 1].clone()
        keep = 0
        for e in prop[:n_acc] + [tok]:  # stop exactly at EOS / n_max, even inside an accepted draft
            new_ids.append(e)
            keep += 1
            if e == eos or len(new_ids) >= n_max:
                break
        step.hidden[step.pos: step.pos + keep].copy_(st["hidden"][:keep])
        amax.extend(va[j: j + 1] for j in range(keep))
        step.resume(keep, st)
    return new_ids, amax, stats
