"""Speculative greedy decoding without a GPU: the Drafter's proposals (longest suffix, template slots, the adaptive back-off) and the
bookkeeping of the generation loop (InteractVLMForCausalLM._generate_speculative) against a scripted stand-in for the language model:
emitted ids, hidden rows, verify passes, EOS inside an accepted draft, the max_new_tokens and max_len caps."""
import torch

from interactvlm_amd import demo
from interactvlm_amd import model as M
from interactvlm_amd.speculative import SLOT, Drafter


# ---- Drafter ------------------------------------------------------------------------------------------------------------------
def test_longest_suffix_wins():
    d = Drafter([[1, 2, 3, 4, 5], [9, 3, 4, 7, 8]])
    assert d.propose([3, 4], 16) == [5]              # (3, 4) first occurs in template 0
    assert d.propose([9, 3, 4], 16) == [7, 8]        # the 3-id suffix beats the 2-id one
    assert d.propose([0, 0, 1, 2, 3, 4], 3) == [5]   # suffixes of at most n = 4 ids; at most k - 1 proposals
    assert d.propose([1, 2, 3], 3) == [4, 5]
    assert d.propose([42], 16) == []                 # no match: nothing
    assert d.propose([5], 16) == []                  # a match at the end of a template has no continuation
    assert d.propose([1], 1) == []


def test_empty_answer_matches_template_starts():
    d = Drafter([[7, 8, 9], [5, SLOT, 6]])
    assert d.propose([], 16) == [7, 8, 9]
    assert Drafter([[SLOT, 4, 5]]).propose([], 16) == []  # (a template that starts with free text has no start to propose)


def test_slot_fragments_and_resume_after_the_slot():
    tmpl = [10, 11, 12, SLOT, 20, 21, 22, 23]
    d = Drafter([tmpl])
    assert d.fragments == [[10, 11, 12], [20, 21, 22, 23]]
    assert d.propose([10], 16) == [11, 12]            # the fragment ends at the slot: no guess across free text
    assert d.propose([10, 11, 12], 16) == []
    assert d.propose([10, 11, 12, 77, 78], 16) == []  # free text
    assert d.propose([10, 11, 12, 77, 78, 20], 16) == [21, 22, 23]  # drafting resumes on the fragment after the slot


def test_adaptive_back_off():
    d = Drafter([[1, 2, 3, 4, 5, 6]])
    assert d.propose([2], 16) == [3, 4, 5, 6]
    d.observe(4, 1)                                  # rejected after one id
    assert d.propose([2, 3, 9], 16) == []            # no match anyway
    assert d.propose([2, 3, 9, 4], 16) == []         # a 1-id match is not enough after a rejection
    assert d.propose([9, 4, 5], 16) == [6]           # a 2-id match is
    d.observe(1, 1)                                  # fully accepted: back to 1-id matches
    assert d.propose([4], 16) == [5, 6]
    nd = Drafter([[1, 2, 3, 4, 5, 6]], adaptive=False)
    nd.observe(4, 0)
    assert nd.propose([4], 16) == [5, 6]


def test_answer_templates_of_the_released_formats():
    class Tok:
        bos_token_id, eos_token_id = 1, 2

        def __init__(self):
            self.vocab = {}

        def __call__(self, text):
            class R:
                input_ids = [1] + [self.vocab.setdefault(w, 10 + len(self.vocab)) for w in text.split()]
            return R

    tok = Tok()
    simple, parts = demo.answer_templates(tok, "hcontact", seg_token_idx=32000)
    v = tok.vocab
    assert simple == [v["Sure,"], 32000, v["."], 2]
    assert parts[:5] == [v[w] for w in "The contacting body parts are".split()] and parts[5] is SLOT
    assert parts[6:] == [v[w] for w in ", and the contact region is".split()] + [32000, v["."], 2]


# ---- the generation loop against a scripted model -------------------------------------------------------------------------------
class _ScriptedLlama:
    """The model's greedy answer is SCRIPT: the row fed at position p predicts new id number p - T0 + 1.  Hidden rows are
    (position, fed id); every fed position is recorded (padded rows of a pass apart, which the kernels never append past max_len)."""
    VERIFY_BUCKETS = (4, 8, 16)

    def __init__(self, script, T0, vocab=64):
        self.script, self.T0, self.vocab = list(script), T0, vocab
        self.fed = []  # (position, id) of every real row
        self.passes = []

    def verify_supported(self):
        return True

    def _pred(self, p):
        s = p - self.T0 + 1
        return self.script[s] if s < len(self.script) else 0

    def logits(self, h):
        out = torch.zeros(h.shape[0], self.vocab)
        for r in range(h.shape[0]):
            out[r, self._pred(int(h[r, 0]))] = 1.0
        return out

    def embed_ids(self, ids):
        return torch.stack([torch.zeros(len(ids)), ids.float()], 1)

    def forward(self, x, pos):
        assert x.shape[0] == 1
        self.fed.append((pos, int(x[0, 1])))
        return torch.tensor([[float(pos), x[0, 1]]])

    def verify_state(self, kb):
        i32 = lambda n: torch.zeros(n, dtype=torch.int32)
        return dict(ids=i32(kb), nd=i32(1), pos=i32(1), n_acc=i32(1), tok=i32(1))

    def verify_pass(self, st):
        pos, kb, nd = int(st["pos"][0]), st["ids"].numel(), int(st["nd"][0])
        ids = st["ids"].tolist()
        self.passes.append((pos, nd))
        self.fed.extend((pos + i, ids[i]) for i in range(nd + 1))
        st["hidden"] = torch.tensor([[float(pos + i), float(ids[i])] for i in range(kb)])
        st["amax"] = torch.tensor([self._pred(pos + i) for i in range(kb)], dtype=torch.int32)
        n = 0
        while n < nd and ids[n + 1] == int(st["amax"][n]):
            n += 1
        st["n_acc"][0], st["tok"][0] = n, int(st["amax"][n])
        st["pos"][0] = pos + n + 1
        return st


class _Fixed:
    """proposes the same ids every round (no back-off)"""

    def __init__(self, ids):
        self.ids = list(ids)

    def propose(self, ids, k):
        return self.ids[: k - 1]


class _Oracle:
    """proposes the script's continuation, wrong from its j-th id on"""

    def __init__(self, script, j=None, wrong=63):
        self.script, self.j, self.wrong = script, j, wrong

    def propose(self, ids, k):
        cont = self.script[len(ids): len(ids) + k - 1]
        if self.j is not None:
            cont = cont[: self.j] + [self.wrong] * (len(cont) - self.j)
        return cont


def _run(monkeypatch, script, draft, n_max, eos=2, T0=5, hidden=2):
    monkeypatch.setattr(M.ops, "argmax", lambda x, bump=None: x.argmax(-1).to(torch.int32))
    llm = _ScriptedLlama(script, T0)
    m = object.__new__(M.InteractVLMForCausalLM)
    m.llm, m.device, m.graph_decode = llm, torch.device("cpu"), False
    hidden_all = torch.full((T0 + n_max, hidden), -1.0)
    last = torch.tensor([[float(T0 - 1), 9.0]])  # the prefill's last row predicts new id 0
    ids = torch.arange(T0)
    out_ids, hid = m._generate_speculative(ids, last, T0, n_max, eos, hidden_all, draft)
    new = out_ids[0, T0:].tolist()
    # bookkeeping that holds for every run: one hidden row per fed id that counts, rows = (position, id fed there)
    assert hid.shape[0] == T0 + len(new) - 1
    for r in range(T0, hid.shape[0]):
        assert hid[r].tolist() == [float(r), float(new[r - T0])]
    assert len(m.last_argmax) == len(new) and [int(a) for a in m.last_argmax] == new
    assert all(p < T0 + n_max for p, _ in llm.fed)  # never past the cache (n_max = max_len - T0 in generate)
    return new, m.last_spec, llm


SCRIPT = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34]


def test_loop_fully_accepted_draft(monkeypatch):
    new, spec, llm = _run(monkeypatch, SCRIPT, _Oracle(SCRIPT), n_max=24)
    assert new == SCRIPT
    # 24 ids: the first from the prefill, a pass of 1 + 15 rows (16 ids), then the 7 left: 6 proposals + the pass's own id
    assert spec["pattern"] == [(15, 15), (6, 6)] and spec["passes"] == 2 and spec["plain_steps"] == 0
    assert [p for p, _ in llm.passes] == [5, 21]


def test_loop_all_wrong_and_partly_right(monkeypatch):
    new, spec, _ = _run(monkeypatch, SCRIPT, _Fixed([63, 63, 63]), n_max=10)
    assert new == SCRIPT[:10]
    assert spec["pattern"] == [(3, 0)] * 6 + [(2, 0), (1, 0)] and spec["accepted"] == 0  # one id per pass
    assert spec["plain_steps"] == 1  # (the last id: nothing left to draft)
    for j in (1, 2, 5):
        new, spec, _ = _run(monkeypatch, SCRIPT, _Oracle(SCRIPT, j=j), n_max=20)
        assert new == SCRIPT[:20]
        assert all(n == min(j, m) for m, n in spec["pattern"]), spec["pattern"]


def test_loop_eos_inside_an_accepted_draft(monkeypatch):
    script = SCRIPT[:6] + [2] + SCRIPT[7:]
    new, spec, _ = _run(monkeypatch, script, _Oracle(script), n_max=24)
    assert new == script[:7] and spec["passes"] == 1  # rows past EOS are dropped
    new, spec, _ = _run(monkeypatch, [2] + SCRIPT, _Oracle(SCRIPT), n_max=24)
    assert new == [2] and spec["passes"] == 0  # EOS straight from the prefill


def test_loop_max_new_tokens_inside_a_draft_and_plain_steps(monkeypatch):
    for n_max in (1, 2, 3, 9):
        new, spec, _ = _run(monkeypatch, SCRIPT, _Oracle(SCRIPT), n_max=n_max)
        assert new == SCRIPT[:n_max]
    new, spec, _ = _run(monkeypatch, SCRIPT, _Fixed([]), n_max=6)  # no proposal: the plain step
    assert new == SCRIPT[:6] and spec["passes"] == 0 and spec["plain_steps"] == 5
    # a draft longer than what is left is cut so that no row is fed at or past T0 + n_max - 1
    new, spec, llm = _run(monkeypatch, SCRIPT, _Fixed(SCRIPT[1:]), n_max=4)
    assert new == SCRIPT[:4] and spec["pattern"] == [(2, 2)]
    assert max(p for p, _ in llm.fed) == 5 + 4 - 2


def test_drafter_through_the_loop(monkeypatch):
    """a template bank with a slot: ids inside the template are drafted, the free text runs plain steps"""
    script = [40, 41, 42, 43, 50, 51, 44, 45, 46, 2]
    tmpl = [40, 41, 42, 43, SLOT, 44, 45, 46, 2]
    new, spec, _ = _run(monkeypatch, script, Drafter([tmpl]), n_max=16)
    assert new == script
    assert spec["pattern"] == [(3, 3), (3, 3)] and spec["plain_steps"] == 2
    never = Drafter([[60, 61, 62]])  # never matches: every step is the plain one
    new, spec, _ = _run(monkeypatch, script, never, n_max=16)
    assert new == script and spec["passes"] == 0 and spec["plain_steps"] == len(script) - 1


def test_generate_keeps_plain_path_without_draft():
    """without a draft generate() takes the existing loop: the signature default is None"""
    import inspect

    for fn in (M.InteractVLMForCausalLM.generate, M.InteractVLMForCausalLM.evaluate):
        assert inspect.signature(fn).parameters["draft"].default is None
    assert "draft" not in inspect.signature(M.InteractVLMForCausalLM.generate_batch).parameters
