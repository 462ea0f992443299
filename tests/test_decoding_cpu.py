"""The greedy decode loop without a GPU (decoding.greedy): a scripted step stands in for the decode step of B = 1 and B = 3 sequences,
forced ids and free-running, sequences that stop at EOS on different steps or at their length cap; and the fused-wait fallback of
generate() against a scripted language model whose captured step reports an expired wait."""
from types import SimpleNamespace

import pytest
import torch

from interactvlm_amd import decoding, llava
from interactvlm_amd import model as M

EOS = 2


class _Event:
    def __init__(self, step):
        self.step, self.k = step, len(step.fed)

    def synchronize(self):
        self.step.syncs.append((self.k, len(self.step.fed)))


class _ScriptedStep:
    """B sequences; the step that consumes id s of sequence b produces script[b][s + 1].  Records every fed row and, per event the
    host waits for, (steps enqueued when it was recorded, steps enqueued when the host waited)."""

    def __init__(self, script):
        self.script = script
        self.fed, self.syncs, self.events = [], [], 0

    def __call__(self, tok, out=None):
        s = len(self.fed)
        self.fed.append(tok.tolist())
        nxt = torch.tensor([sc[s + 1] for sc in self.script], dtype=torch.int32)
        return nxt if out is None else out.copy_(nxt)

    def event(self):
        self.events += 1
        return _Event(self)


def _expected(src, n_seq):
    out = []
    for ids, n in zip(src, n_seq):
        ids = ids[:n]
        out.append(ids[: ids.index(EOS) + 1] if EOS in ids else ids)
    return out


SCRIPTS = [
    # B = 1: EOS as the first id, EOS later, no EOS (the length cap), a single id
    ([[EOS, 5, 6, 7, 8, 9]], [6]),
    ([[11, 12, 13, EOS, 15, 16, 17]], [7]),
    ([[11, 12, 13, 14, 15, 16, 17]], [7]),
    ([[11, 12]], [1]),
    # B = 3: stops at different steps, one at its own (shorter) cap, one never before the common cap
    ([[11, EOS, 13, 14, 15, 16, 17, 18], [21, 22, 23, 24, EOS, 26, 27, 28], [31, 32, 33, 34, 35, 36, 37, 38]], [8, 8, 5]),
    ([[11, 12, 13, 14, 15, 16, 17, 18], [21, EOS, 23, 24, 25, 26, 27, 28], [EOS, 32, 33, 34, 35, 36, 37, 38]], [8, 8, 8]),
    ([[EOS, 12, 13], [EOS, 22, 23], [31, EOS, 33]], [3, 3, 3]),
]


@pytest.mark.parametrize("script,n_seq", SCRIPTS)
def test_greedy_free_running(script, n_seq):
    step = _ScriptedStep(script)
    nxt = torch.tensor([sc[0] for sc in script], dtype=torch.int32)
    new, amax = decoding.greedy(step, nxt, n_seq, EOS)
    want = _expected(script, n_seq)
    assert new == want
    n_max, last = max(n_seq), max(len(w) for w in want)
    # every step fed the previous step's argmax (finished sequences keep stepping)
    assert step.fed == [[sc[s] for sc in script] for s in range(len(step.fed))]
    # exactly one step past the id the last sequence stops on (none past n_max - 1 steps)
    assert len(step.fed) == min(last, n_max - 1)
    # the host waits for id s - 1 with the step of id s already queued: one replay ahead, except after the last step
    assert [k for k, _ in step.syncs] == list(range(last))
    assert all(q == min(k + 1, n_max - 1) for k, q in step.syncs), step.syncs
    assert len(amax) == last and [a.tolist() for a in amax] == [[sc[s] for sc in script] for s in range(last)]


@pytest.mark.parametrize("script,n_seq", SCRIPTS)
def test_greedy_forced(script, n_seq):
    B, n_max = len(script), max(n_seq)
    forced_ids = [[100 + 10 * b + s for s in range(n_max)] for b in range(B)]
    for b, sc in enumerate(script):  # the forced ids carry the script's EOS positions
        forced_ids[b] = [EOS if sc[s] == EOS else forced_ids[b][s] for s in range(n_max)]
    forced_dev = torch.tensor(forced_ids, dtype=torch.int32).t().contiguous()
    step = _ScriptedStep(script)
    nxt = torch.tensor([sc[0] for sc in script], dtype=torch.int32)
    new, amax = decoding.greedy(step, nxt, n_seq, EOS, forced=(forced_ids, forced_dev))
    want = _expected(forced_ids, n_seq)
    assert new == want
    last = max(len(w) for w in want)
    assert step.fed == [[f[s] for f in forced_ids] for s in range(last - 1)]  # no step past the last id
    assert step.events == 0 and step.syncs == []  # never a wait on the device
    assert [a.tolist() for a in amax] == [[sc[s] for sc in script] for s in range(last)]  # the argmax is still computed


# ---- the fused-wait fallback of generate() -----------------------------------------------------------------------------------
class _FusedLlama(llava.Llama):
    """The prompt's last row predicts SCRIPT[0], the row fed at position p SCRIPT[p - T0 + 1]; hidden rows are (position, fed id).
    Its captured step has the fused attention + o_proj launch while fuse_attn_oproj is on, and then every wait expires."""
    K = llava._GraphKey
    device = torch.device("cpu")

    def __init__(self, script, T0):
        self.script, self.T0, self.max_len, self.fuse_attn_oproj = script, T0, 64, True
        self.prefills, self.generations = 0, []
        self._graphs = {self.K(False, 1, "f16", True, False, True): "fused step",
                        self.K(False, 1, "f16", True, False, False): "two-launch step",
                        self.K(True, 4, "f16", True, False, False): "batched step"}

    def verify_supported(self):
        return True

    def forward(self, x, pos0):
        self.prefills += 1
        return torch.tensor([[float(pos0 + i), 0.0] for i in range(x.shape[0])])

    def logits(self, h):
        out = torch.zeros(h.shape[0], 64)
        for r in range(h.shape[0]):
            s = int(h[r, 0]) - self.T0 + 1
            out[r, self.script[s] if s < len(self.script) else 0] = 1.0
        return out

    def decode_graph(self, pos):
        i32 = lambda v: torch.tensor([v], dtype=torch.int32)
        st = dict(tok=i32(0), pos=i32(pos), pos64=torch.tensor([pos]))
        if self.fuse_attn_oproj:
            st["fused"] = dict(step=i32(0), counters=torch.zeros(2, 32, dtype=torch.int32), status=i32(0))

        def replay():
            h = torch.tensor([[float(st["pos"][0]), float(st["tok"][0])]])
            st["hidden"], st["nxt"] = h, M.ops.argmax(self.logits(h))
            st["pos"] += 1
            if "fused" in st:
                st["fused"]["status"].fill_(1)  # a bounded wait expired

        st["graph"] = SimpleNamespace(replay=replay)
        self.generations.append(st)
        return st


class _NoDraft:
    def __init__(self):
        self.calls = 0

    def propose(self, ids, k):
        self.calls += 1
        return []


@pytest.mark.parametrize("mode", ["forced", "free", "draft"])
def test_expired_fused_wait_redoes_the_generation_on_the_two_launch_path(monkeypatch, mode):
    monkeypatch.setattr(M.ops, "argmax", lambda x, bump=None: x.argmax(-1).to(torch.int32))
    monkeypatch.setattr(M.graphs, "enabled", lambda flag, *t: bool(flag))
    monkeypatch.setattr(decoding._Step, "event", lambda self: SimpleNamespace(synchronize=lambda: None))
    T0, script = 5, [11, 12, 13, EOS, 15, 16]
    llm = _FusedLlama(script, T0)
    m = object.__new__(M.InteractVLMForCausalLM)
    m.llm, m.device, m.graph_decode = llm, torch.device("cpu"), True
    m.config = SimpleNamespace(llama=SimpleNamespace(hidden=2))
    m.encode_images = lambda ic: torch.zeros(1, 1, 2)
    m._input_embeds = lambda ids, feats: torch.zeros(T0, 2)
    prefilled = []
    draft = _NoDraft() if mode == "draft" else None
    forced = [31, 32, 33, 34] if mode == "forced" else None
    out_ids, hidden = m.generate(None, torch.arange(3)[None], 6, EOS, forced, after_prefill=lambda: prefilled.append(1), draft=draft)
    new = forced or script[:4]
    assert out_ids[0].tolist() == [0, 1, 2] + new
    assert hidden.shape[0] == T0 + len(new) - 1
    assert hidden[T0:].tolist() == [[float(T0 + i), float(new[i])] for i in range(len(new) - 1)]
    # the first generation ran on the fused step, its wait expired: the fused step is dropped for good, the call redone once
    assert len(llm.generations) == 2 and "fused" in llm.generations[0] and "fused" not in llm.generations[1]
    assert llm.fuse_attn_oproj is False and not any(k.fused for k in llm._graphs) and len(llm._graphs) == 2
    assert llm.prefills == 2 and prefilled == [1]  # (the SAM encoder that after_prefill enqueued is not enqueued twice)
    assert m.last_spec is None if draft is None else m.last_spec["plain_steps"] == len(new) - 1
    if draft is not None:
        assert draft.calls == 2 * (len(new) - 1)  # the redo decodes with the draft again
