"""In-flight batching: greedy decoding of MANY prompts against ONE resident video over a fixed set of text-cache slots.

A decode step costs almost the same for 1 row as for 16 (it streams the video's K/V and the weights whatever the row count), so the
throughput of a many-questions workload is the number of LIVE rows per step.  `generate()` decodes a static batch: it ends when its longest
row ends, and finished rows keep their place.  Here a finished prompt frees its slot at once and the next waiting prompt takes it; every
decode step carries live rows only, each at its own cache position.

Host logic only, engine-agnostic (no torch import): the engine supplies
    max_inflight_rows() -> int
    new_text_slots(S, Lmax) -> slots object with a host list `length` (-1 = free)
    slots_prefill(slots, slot_ids, prompts, mm) -> last hidden [n, H]     admits n prompts (lists of text ids) into n free slots
    slots_decode(slots, slot_ids, token_ids, mm) -> hidden [M, H]         one step for the M listed slots
    logits_argmax(hidden) -> (logits, ids)
    token_logprobs(hidden) -> (ids, logprob, rank)                        only with `logprobs=True`: the greedy token's log-probability
`vidi_amd.engine.VidiEngine` implements them with HIP kernels; tests/test_inflight.py drives this loop with a scripted fake and with the CPU
oracle."""
from __future__ import annotations

from collections import deque
from typing import Callable, List, Optional, Sequence

SLOT_METHODS = ("new_text_slots", "slots_prefill", "slots_decode")


def _ids(idx) -> List[int]:
    return [int(t) for t in (idx.tolist() if hasattr(idx, "tolist") else idx)]


def _ids_logprobs(ids, lp):
    """the ids and their log-probabilities on the host.  Device tensors come over in ONE copy: fp64 holds an id and an fp32 value exactly"""
    if hasattr(ids, "double") and hasattr(lp, "double"):
        import torch
        both = torch.stack((ids.double(), lp.double())).tolist()
        return [int(t) for t in both[0]], both[1]
    return _ids(ids), [float(x) for x in (lp.tolist() if hasattr(lp, "tolist") else lp)]


def run_inflight(engine, prompts: Sequence[Sequence[int]], mm, max_new: Sequence[int], eos_ids: Sequence[int] = (),
                 max_rows: Optional[int] = None, min_admit: int = 2,
                 on_finish: Optional[Callable[[int, List[int]], None]] = None, logprobs: bool = False):
    """prompts[i]: text ids (no placeholder); max_new[i] >= 1.  Returns, in input order, every prompt's new tokens up to and including its
    first EOS, or max_new[i] of them.

    Each iteration: (1) admission — while a slot is free and a prompt waits, and at least min(min_admit, waiting) slots are free or no row
    is live, ALL free slots are filled through one `slots_prefill` call; a prompt's first token comes from its prefill logits, and a prompt
    that is complete after it (EOS, max_new == 1) gives its slot back without ever occupying a decode row — the rule is then applied
    again, so with min_admit = 1 no slot idles while a prompt waits (the default is 2: on the measured workload, profiles/inflight_queries.json,
    pairing admissions halves the prefill calls and wins 1.7 % over 1; 4 loses); (2) one `slots_decode` over the live rows, `logits_argmax`, one D2H
    copy of the ids; (3) finished rows free their slot.

    `logprobs=True`: both places that call `logits_argmax` call `engine.token_logprobs(hidden)` instead (the same argmax over the same logits,
    plus the chosen token's log-probability; ids and values still come over in one D2H copy per step) and the result is (tokens, logprobs):
    logprobs[i][j] is the log-probability of tokens[i][j], the EOS token's included."""
    n = len(prompts)
    if len(max_new) != n or any(int(m) < 1 for m in max_new):
        raise ValueError("max_new: one count >= 1 per prompt")
    if n == 0:
        return ([], []) if logprobs else []
    S = int(max_rows if max_rows is not None else engine.max_inflight_rows())
    if S < 1 or int(min_admit) < 1:
        raise ValueError(f"max_rows = {S}, min_admit = {min_admit}: both at least 1")
    eos = {int(e) for e in eos_ids}
    slots = engine.new_text_slots(S, max(len(p) for p in prompts) + max(int(m) for m in max_new))
    free = list(range(S))                                  # ascending: the lowest free slot is taken first
    waiting = deque(range(n))
    live = {}                                              # slot -> prompt index
    last = {}                                              # slot -> the token decided last (not in the cache yet)
    out: List[List[int]] = [[] for _ in range(n)]
    lps: List[List[float]] = [[] for _ in range(n)]

    def decide(hid):
        """-> the greedy token of every row (and, with `logprobs`, its log-probability)"""
        if not logprobs:
            toks = _ids(engine.logits_argmax(hid)[1])
            return toks, [None] * len(toks)
        ids, lp = engine.token_logprobs(hid)[:2]
        return _ids_logprobs(ids, lp)

    def emit(i: int, tok: int, lp=None) -> bool:
        out[i].append(tok)
        if lp is not None:
            lps[i].append(lp)
        done = tok in eos or len(out[i]) >= int(max_new[i])
        if done and on_finish is not None:
            on_finish(i, list(out[i]))
        return done

    def release(s: int) -> None:
        slots.length[s] = -1
        live.pop(s, None)
        last.pop(s, None)
        free.append(s)
        free.sort()

    while waiting or live:
        while waiting and free and (len(free) >= min(int(min_admit), len(waiting)) or not live):
            k = min(len(free), len(waiting))
            sl = [free.pop(0) for _ in range(k)]
            idx = [waiting.popleft() for _ in range(k)]
            hid = engine.slots_prefill(slots, sl, [list(prompts[i]) for i in idx], mm)
            for s, i, tok, lp in zip(sl, idx, *decide(hid)):
                live[s] = i
                if emit(i, tok, lp):
                    release(s)
                else:
                    last[s] = tok
        if not live:
            continue
        sl = sorted(live)
        hid = engine.slots_decode(slots, sl, [last[s] for s in sl], mm)
        for s, tok, lp in zip(sl, *decide(hid)):                            # one D2H copy per step, like the plain loop
            if emit(live[s], tok, lp):
                release(s)
            else:
                last[s] = tok
    return (out, lps) if logprobs else out


def simulate_steps(lengths: Sequence[int], max_rows: int, min_admit: int = 2):
    """The loop's step-count model for answers of known lengths (no EOS): -> (decode steps, sum of live rows over the steps, prefill calls).
    A prompt of length 1 takes no decode row; one of length n takes n - 1."""
    free, waiting, live = max_rows, deque(int(x) for x in lengths), []
    steps = rows = prefills = 0
    while waiting or live:
        while waiting and free and (free >= min(min_admit, len(waiting)) or not live):
            k = min(free, len(waiting))
            prefills += 1
            for _ in range(k):
                left = waiting.popleft() - 1
                if left > 0:
                    live.append(left)
                    free -= 1
        if not live:
            continue
        steps += 1
        rows += len(live)
        live = [x - 1 for x in live]
        free += sum(1 for x in live if x == 0)
        live = [x for x in live if x > 0]
    return steps, rows, prefills


def static_batch_steps(lengths: Sequence[int], batch: int):
    """What successive `generate()` calls of `batch` prompts in input order cost: every batch decodes until its longest answer ends
    -> (decode steps, sum of rows over the steps, prefill calls); a batch's rows all stay in the step until the batch ends."""
    steps = rows = calls = 0
    for i in range(0, len(lengths), batch):
        chunk = [int(x) for x in lengths[i: i + batch]]
        steps += max(chunk) - 1
        rows += (max(chunk) - 1) * len(chunk)
        calls += 1
    return steps, rows, calls
