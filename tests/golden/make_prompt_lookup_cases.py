"""Writes prompt_lookup_cases.json: what transformers' `PromptLookupCandidateGenerator.get_candidates` proposes for ~200 small histories
(the rule vidi_amd/spec.py::lookup_draft restates).  Run with transformers installed:  python tests/golden/make_prompt_lookup_cases.py"""
import json
import os
import random

import torch


def hf_draft(history, num_tokens, max_ngram, eos_ids):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    eos = torch.tensor(eos_ids, dtype=torch.int64) if eos_ids else None
    gen = PromptLookupCandidateGenerator(eos_token_id=eos, num_output_tokens=num_tokens, max_matching_ngram_size=max_ngram, max_length=1 << 30)
    ids = torch.tensor([history], dtype=torch.int64)
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(history):].tolist()


def random_case(rng):
    vocab = rng.choice([3, 5, 9])
    n = rng.randint(1, 40)
    eos = rng.sample(range(vocab), rng.choice([0, 1, 2]))
    return dict(history=[rng.randrange(vocab) for _ in range(n)], num_tokens=rng.choice([1, 3, 7, 10, 15]), max_ngram=rng.randint(1, 4), eos=eos)


HAND = [
    # (the trailing n-gram always matches itself, with an empty continuation: "no match" and "match only at the tail" are one case)
    dict(name="no match but the tail itself (empty continuation)", history=[1, 2, 3, 4, 5], num_tokens=3, max_ngram=2, eos=[]),
    dict(name="earlier match that ends at the last token", history=[4, 4], num_tokens=3, max_ngram=1, eos=[]),
    dict(name="2-gram only at the tail, 1-gram earlier", history=[1, 2, 3, 3], num_tokens=2, max_ngram=2, eos=[]),
    dict(name="EOS as first candidate", history=[1, 2, 0, 5, 1, 2], num_tokens=3, max_ngram=2, eos=[0]),
    dict(name="EOS in the middle", history=[1, 2, 6, 0, 5, 1, 2], num_tokens=4, max_ngram=2, eos=[0]),
    dict(name="history of length 1", history=[3], num_tokens=3, max_ngram=2, eos=[]),
    dict(name="clipped at the end of the history", history=[7, 8, 9, 7, 8], num_tokens=10, max_ngram=2, eos=[]),
    dict(name="first match wins over a longer later one", history=[1, 2, 9, 1, 2, 3, 4, 5, 1, 2], num_tokens=4, max_ngram=2, eos=[]),
    dict(name="falls back to the 1-gram", history=[5, 1, 6, 7, 2, 1], num_tokens=2, max_ngram=3, eos=[]),
]


if __name__ == "__main__":
    import transformers
    rng = random.Random(20)
    cases = [dict(c) for c in HAND]
    while len(cases) < 200:
        cases.append(dict(name=f"random {len(cases)}", **random_case(rng)))
    for c in cases:
        c["draft"] = hf_draft(c["history"], c["num_tokens"], c["max_ngram"], c["eos"])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prompt_lookup_cases.json")
    with open(out, "w") as f:
        src = f"transformers {transformers.__version__} PromptLookupCandidateGenerator.get_candidates, max_length = 2^30"
        f.write('{"source": ' + json.dumps(src) + ',\n"cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")      # one case per line
    print(out, len(cases), "cases,", sum(bool(c["draft"]) for c in cases), "with a draft")
