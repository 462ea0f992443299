"""Draft proposals for speculative greedy decoding ("prompt lookup" against answer templates).

The released checkpoints answer in fixed templates ("Sure, [SEG].", "The contacting body parts are {body_parts}, and the contact
region is [SEG]."), so most answer tokens are known in advance.  ``InteractVLMForCausalLM.generate(..., draft=Drafter(...))`` feeds
the last emitted token plus up to 15 proposed ones through ONE pass over the weights (``Llama.verify_step``) and keeps the leading
proposals that equal the model's own argmax: every emitted id is still the argmax of the model's logits (greedy-exact), a wrong
proposal only costs the extra rows of that pass.

Pure Python; the token ids come from the caller (``demo.answer_templates`` builds the two released formats).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

SLOT = None  # a free-text slot inside a template ({body_parts}): drafting resumes on the fragment after it


class Drafter:
    """Proposes the continuation of the longest suffix (up to ``n`` ids) of the generated ids that occurs in a template.

    templates: token-id sequences; an entry ``SLOT`` (None) marks free text and splits the template into fragments that are matched
    on their own.  An empty answer matches the start of every template (the first template's start is proposed).
    adaptive: after a rejected proposal nothing is proposed until the suffix match is at least ``min_match_after_reject`` ids long,
    so a model that ignores the templates pays almost nothing.
    """

    def __init__(self, templates: Sequence[Sequence[Optional[int]]], n: int = 4, adaptive: bool = True,
                 min_match_after_reject: int = 2):
        self.fragments: List[List[int]] = []
        self.starts: List[List[int]] = []  # the fragment each template starts with
        for t in templates:
            cur: List[int] = []
            frags = []
            for tok in t:
                if tok is SLOT:
                    frags.append(cur)
                    cur = []
                else:
                    cur.append(int(tok))
            frags.append(cur)
            frags = [f for f in frags if f]
            if frags and t and t[0] is not SLOT:
                self.starts.append(frags[0])
            self.fragments.extend(frags)
        self.n = int(n)
        self.adaptive = adaptive
        self.min_match_after_reject = int(min_match_after_reject)
        self.backed_off = False
        self.last_match = 0  # length of the suffix match behind the last proposal (0: none / template start)

    def reset(self):
        self.backed_off = False
        self.last_match = 0

    def _lookup(self, ids: Sequence[int]):
        """-> (match length, continuation) for the longest suffix of ids (<= n ids) found inside a fragment with at least one id
        after it; the first occurrence in template order wins."""
        for m in range(min(self.n, len(ids)), 0, -1):
            suf = list(ids[len(ids) - m:])
            for f in self.fragments:
                for s in range(len(f) - m):
                    if f[s: s + m] == suf:
                        return m, f[s + m:]
        return 0, []

    def propose(self, ids: Sequence[int], k: int) -> List[int]:
        """up to k - 1 draft ids to follow ``ids`` (the answer generated so far)"""
        if k <= 1:
            return []
        if len(ids) == 0:
            m, cont = 0, (self.starts[0] if self.starts else [])
        else:
            m, cont = self._lookup(ids)
        self.last_match = m
        if self.adaptive and self.backed_off and m < self.min_match_after_reject:
            return []
        return list(cont[: k - 1])

    def observe(self, n_proposed: int, n_accepted: int):
        """the outcome of the last proposal (called by the generation loop after each verify pass)"""
        if n_proposed > 0:
            self.backed_off = n_accepted < n_proposed
