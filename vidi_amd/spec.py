"""Prompt-lookup speculative decoding, host side: where the drafts come from and which of them a verify step keeps.

HF reaches this through `generate(prompt_lookup_num_tokens=K, max_matching_ngram_size=N)` (the reference forwards `**kwargs` to HF's
generate(), gemma.py:646-655): the continuation of the latest n-gram found earlier in the sequence is proposed as the next tokens, and
one forward over `[last token, drafts]` checks them all.  Pure Python on lists of ints: no torch, no device work."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple


def lookup_draft(history: Sequence[int], num_tokens: int, max_ngram: int, eos_ids: Iterable[int] = ()) -> List[int]:
    """The rule of HF's `PromptLookupCandidateGenerator.get_candidates` (without its `max_length` clip and logits processors, which the
    caller handles by bounding `num_tokens`): n-gram sizes min(max_ngram, len - 1) .. 1; for each, the matches of the trailing n-gram from
    left to right; the FIRST match with a non-empty continuation wins, whatever the size of later ones.  The continuation holds at most
    `num_tokens` tokens, stops at the end of the history and in front of the first EOS id (so an EOS as first candidate gives no draft,
    and no smaller n-gram is tried then — HF's behaviour).  [] means "no draft"."""
    if num_tokens <= 0 or max_ngram <= 0:
        raise ValueError("Invalid max_matching_ngram_size or num_output_tokens")                   # HF's own check
    h = list(history)
    n = len(h)
    eos = set(int(e) for e in eos_ids)
    for size in range(min(max_ngram, n - 1), 0, -1):
        tail = h[n - size:]
        for at in range(n - size + 1):
            if h[at: at + size] != tail:
                continue
            start = at + size
            end = min(start + num_tokens, n)
            if start < end:
                out = []
                for t in h[start:end]:
                    if t in eos:
                        break
                    out.append(t)
                return out
    return []


def accept_run(argmax: Sequence[int], draft: Sequence[int], eos_ids: Iterable[int], room: int) -> Tuple[int, List[int]]:
    """What a verify step yields.  `argmax[i]` is the model's next token after consuming input i of `[last_token, d_0 .. d_{k-1}]`.
    n_accept = the number of leading i with argmax[i] == d_i; the step emits d_0 .. d_{a-1} and then argmax[a] (the model's own token at
    the first disagreement, or the bonus token when every draft held) — exactly the tokens plain greedy decoding would have produced one
    by one.  The run is cut after the first EOS and at `room`, the number of tokens still allowed.  -> (n_accept, emitted)"""
    if len(argmax) != len(draft) + 1:
        raise ValueError(f"{len(argmax)} verify rows for {len(draft)} drafts: one row per draft and one for the last token")
    a = 0
    while a < len(draft) and int(argmax[a]) == int(draft[a]):
        a += 1
    eos = set(int(e) for e in eos_ids)
    emitted: List[int] = []
    for t in list(draft[:a]) + [argmax[a]]:
        if len(emitted) >= room:
            break
        emitted.append(int(t))
        if int(t) in eos:
            break
    return a, emitted
