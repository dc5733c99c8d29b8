"""Writes generate_engine_calls.json: for a handful of small calls of `generate()` / `generate_inflight()` / `score()` over the CPU oracle
engines, EVERY engine method the product class calls (name + a summary of the arguments) and what the call returned.  The engine calls decide
the GPU launches, so a change of vidi_amd/model.py that leaves this file as it is leaves the launches as they are.

The expected values belong to the commit BEFORE the change under test: run this script on a checkout of that commit and commit its output,

    python tests/golden/make_generate_engine_calls.py [OUT.json]

(only the public entry points and the `_spec_draft` seam are used, so the same script runs on either side of a refactor).
tests/test_generate_engine_calls.py imports `run_case` from here and compares."""
import inspect
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "oracle"), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "generate_engine_calls.json")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------------------------
def summary(x):
    """an argument as JSON: tensors by shape and dtype (small integer tensors — token ids, positions, masks — with their values), numbers as
    they are, lists by length (short lists of ints with their values), a text state by its counters, other objects by their type's name"""
    if torch.is_tensor(x):
        d = {"shape": list(x.shape), "dtype": str(x.dtype).replace("torch.", "")}
        if not x.is_floating_point() and x.numel() <= 64:
            d["values"] = x.reshape(-1).long().tolist()
        return d
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, (list, tuple)):
        d = {"len": len(x)}
        if len(x) <= 64 and all(isinstance(v, int) for v in x):
            d["values"] = list(x)
        return d
    if hasattr(x, "n_valid") and hasattr(x, "past_len"):
        return {"text_state": {"B": x.B, "Lmax": x.Lmax, "past_len": x.past_len, "n_valid": None if x.n_valid is None else x.n_valid.tolist()}}
    return type(x).__name__


class Recorder:
    """stands in front of an oracle engine: attributes read and written go to the engine, and every method called THROUGH the recorder is
    logged with its arguments under the parameter names of the engine's method (what an engine method calls on itself is not a call of the
    product class and is not logged)"""

    def __init__(self, engine):
        object.__setattr__(self, "_engine", engine)
        object.__setattr__(self, "log", [])

    def __getattr__(self, name):
        attr = getattr(self._engine, name)                              # AttributeError here keeps `hasattr` truthful
        if not inspect.ismethod(attr):
            return attr

        def call(*args, **kwargs):
            given = inspect.signature(attr).bind(*args, **kwargs).arguments
            entry = {"call": name}
            for k, v in given.items():
                if k == "kw" and isinstance(v, dict):                   # the encoders' **kw
                    entry.update({kk: summary(vv) for kk, vv in sorted(v.items())})
                else:
                    entry[k] = summary(v)
            self.log.append(entry)
            return attr(*args, **kwargs)
        return call

    def __setattr__(self, name, value):
        setattr(self._engine, name, value)


def plain(x):
    """a returned value as JSON (floats rounded to 1e-6: compared with a tolerance, see the test)"""
    if torch.is_tensor(x):
        v = x.detach().cpu()
        if not v.is_floating_point():
            return v.tolist()
        return [[None if not torch.isfinite(t) else round(float(t), 6) for t in r] for r in v.reshape(-1, v.shape[-1])] if v.dim() > 1 else \
            [round(float(t), 6) for t in v]
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, float):
        return round(x, 6)
    if x is None or isinstance(x, (bool, int, str)):
        return x
    return {k: plain(v) for k, v in sorted(vars(x).items())}            # SimpleNamespace, CandidateScore


# ---------------------------------------------------------------------------------------------------------------------------------------
# one tiny model, four engines over the same weights
# ---------------------------------------------------------------------------------------------------------------------------------------
SEED = 4                                                            # tests/test_spec_decode.py's: an untied head, so the tokens of a run vary
PROMPT = [2, 21, 22, -200, 23, 24, 25, 21, 22]
RAGGED = [[2, 21, 22, -200, 23, 24, 25], [2, 30, -200, 31, 0, 0, 0], [2, 40, 41, 42, 43, 0, 0]]
RAGGED_MASK = [[1] * 7, [1] * 4 + [0] * 3, [1] * 5 + [0] * 2]
LEFT = [[0, 0, 0, 2, 30, -200, 31], [2, 21, 22, -200, 23, 24, 25]]
LEFT_MASK = [[0] * 3 + [1] * 4, [1] * 7]
INFLIGHT = [[2, 21, 22], [2, 30, -200, 31, 32, 33], list(range(40, 49)), [2, 50, 51, 52], [2, 60]]
INFLIGHT_NEW = [4, 1, 3, 5, 2]
CANDIDATES = [[7], [8, 9, 10], [11, 12, 13, 14, 15, 16]]
_env = {}


def env():
    if not _env:
        from oracle_engine import OracleEngine
        from test_inflight import InflightOracleEngine
        from test_score import ScoreOracleEngine
        from test_spec_decode import SpecOracleEngine
        from util import seeded
        from vidi_amd.config import tiny
        from vidi_amd.model import VidiForCausalLM
        from vidi_amd.weights import init_random_weights
        cfg = tiny(tie_word_embeddings=False)
        w = init_random_weights(cfg, seed=SEED, dtype=torch.float32, device="cpu")
        S = cfg.vis_image_size
        e = SimpleNamespace(cfg=cfg, rec={}, model={}, inner={})
        for name, cls in (("plain", OracleEngine), ("spec", SpecOracleEngine), ("inflight", InflightOracleEngine), ("score", ScoreOracleEngine)):
            e.inner[name] = cls(cfg, w)
            e.rec[name] = Recorder(e.inner[name])
            e.model[name] = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=e.rec[name])
        e.direct = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=e.inner["spec"])      # the same engine, not recorded
        e.images = [seeded((2, 3, S, S), 702, 0.5).clamp(-1, 1), seeded((3, 3, S, S), 703, 0.5).clamp(-1, 1)]
        e.audios = [seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 710, 0.3), seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 711, 0.3)]
        e.mm = e.direct.encode_mm_state(e.images[0][None], e.audios[0][None], [100])       # the oracle's video state is the same object for every engine
        _env.update(e=e)
    return _env["e"]


def T(rows):
    return torch.tensor(rows, dtype=torch.int64)


def case_ragged_right_padded_eos(e):
    """3 right-padded prompts; row 1's second token is declared EOS, so that row stops (and is padded) while the others go on"""
    return e.model["plain"].generate(T(RAGGED), attention_mask=T(RAGGED_MASK), mm_state=e.mm, max_new_tokens=5, eos_token_id=[999999, RAGGED_EOS],
                                     pad_token_id=0)


def case_sample_two_returns(e):
    return e.model["plain"].generate(T([PROMPT]), mm_state=e.mm, do_sample=True, num_return_sequences=2, temperature=0.8, top_k=12, max_new_tokens=4,
                                     eos_token_id=999999, generator=torch.Generator().manual_seed(11))


def case_beams(e):
    return e.model["plain"].generate(T([PROMPT]), mm_state=e.mm, num_beams=3, num_return_sequences=2, max_new_tokens=4, eos_token_id=999999, pad_token_id=0,
                                     return_dict_in_generate=True, output_scores=True)


def case_left_padded(e):
    return e.model["plain"].generate(T(LEFT), attention_mask=T(LEFT_MASK), mm_state=e.mm, max_new_tokens=3, eos_token_id=999999, pad_token_id=0)


def case_two_videos_row_by_row(e):
    old = os.environ.get("VIDI_MULTI_VIDEO")
    os.environ["VIDI_MULTI_VIDEO"] = "0"
    try:
        return e.model["plain"].generate(T(RAGGED[:2]), attention_mask=T(RAGGED_MASK[:2]), images=e.images, audios=e.audios, audio_sizes=[100, 80],
                                         max_new_tokens=3, eos_token_id=999999, pad_token_id=0)
    finally:
        os.environ.pop("VIDI_MULTI_VIDEO")
        if old is not None:
            os.environ["VIDI_MULTI_VIDEO"] = old


def case_prompt_lookup_partly_rejected(e):
    """forced drafts: the plain run's own continuation with the SECOND token of every draft wrong -> one draft accepted, two rolled back"""
    n_new, n_prompt = 9, len(PROMPT) - 1
    want = e.direct.generate(T([PROMPT]), mm_state=e.mm, max_new_tokens=n_new, eos_token_id=999999)[0].tolist()

    def draft(history, k, max_ngram, eos_ids):
        at = len(history) - n_prompt
        return [(t + 1) % e.cfg.vocab_size if i == 1 else t for i, t in enumerate(want[at: at + k])]
    model = e.model["spec"]
    model._spec_draft = draft
    try:
        got = model.generate(T([PROMPT]), mm_state=e.mm, max_new_tokens=n_new, eos_token_id=999999, prompt_lookup_num_tokens=3)
    finally:
        del model._spec_draft
    assert got[0].tolist() == want
    return got


def case_inflight_logprobs(e):
    return e.model["score"].generate_inflight(INFLIGHT, mm_state=e.mm, max_new_tokens=INFLIGHT_NEW, eos_token_id=999999, max_rows=2, min_admit=1,
                                              output_logprobs=True)


def case_score_two_groups(e):
    """rows x padded length <= 22: candidates of 1 and 3 tokens share a call, the 6-token one gets its own; then the torch path of an engine
    without `token_logprobs`"""
    a = e.model["score"].score(PROMPT, CANDIDATES, mm_state=e.mm, max_positions=22)
    b = e.model["plain"].score(T(PROMPT), [T(c) for c in CANDIDATES], mm_state=e.mm, max_positions=22)
    return [a, b]


def case_return_dict_scores_and_hooks(e):
    """greedy with `max_length`, a logits processor (token 5 forbidden), a stopping criterion (row stops after 3 tokens) and the step records"""
    def no_five(input_ids, scores):
        scores = scores.clone()
        scores[:, 5] = float("-inf")
        return scores
    return e.model["plain"].generate(T([PROMPT]), mm_state=e.mm, max_length=len(PROMPT) - 1 + 6, eos_token_id=999999, pad_token_id=0,
                                     logits_processor=[no_five], stopping_criteria=[lambda input_ids, scores: input_ids.shape[1] >= 3],
                                     return_dict_in_generate=True, output_scores=True, output_logits=True)


def refusals(e):
    """(name, thunk): every entry point's refusals, and calls to which several apply (the first one in the order of the checks is raised)"""
    from vidi_amd.engine import MMBatchState
    batch = MMBatchState.__new__(MMBatchState)
    gen, spec, infl, score = e.model["plain"].generate, e.model["spec"].generate, e.model["score"].generate_inflight, e.model["score"].score
    ids = T([PROMPT])
    return [
        ("generate: unsupported keyword", lambda: gen(ids, mm_state=e.mm, max_new_tokens=2, typical_p=0.5, do_sample=True)),
        ("generate: inputs_embeds first", lambda: gen(ids, mm_state=e.mm, inputs_embeds=1, typical_p=0.5)),
        ("generate: num_return_sequences", lambda: gen(ids, mm_state=e.mm, max_new_tokens=2, num_return_sequences=2)),
        ("generate: max_length", lambda: gen(ids, mm_state=e.mm, max_length=3)),
        ("generate: resident batch state, beams", lambda: gen(ids, mm_state=batch, max_new_tokens=2, num_beams=2)),
        ("lookup: bad K", lambda: spec(ids, mm_state=e.mm, max_new_tokens=2, prompt_lookup_num_tokens=-1)),
        ("lookup: two rows", lambda: spec(ids.repeat(2, 1), mm_state=e.mm, max_new_tokens=2, prompt_lookup_num_tokens=3)),
        ("lookup: batch state before hooks", lambda: spec(ids, mm_state=batch, max_new_tokens=2, prompt_lookup_num_tokens=3, do_sample=True)),
        ("lookup: hooks before sharded", lambda: sharded(e, "spec", lambda: spec(ids, mm_state=e.mm, max_new_tokens=2, prompt_lookup_num_tokens=3, do_sample=True,
                                                                                  num_beams=2, logits_processor=[len], stopping_criteria=[len],
                                                                                  return_dict_in_generate=True))),
        ("lookup: sharded", lambda: sharded(e, "spec", lambda: spec(ids, mm_state=e.mm, max_new_tokens=2, prompt_lookup_num_tokens=3))),
        ("lookup: engine without roll-back", lambda: gen(ids, mm_state=e.mm, max_new_tokens=2, prompt_lookup_num_tokens=3)),
        ("inflight: unsupported keyword first", lambda: infl(INFLIGHT, mm_state=batch, typical_p=0.5, do_sample=True)),
        ("inflight: hooks before batch state", lambda: infl(INFLIGHT, mm_state=batch, do_sample=True, num_beams=2, return_dict_in_generate=True,
                                                            prompt_lookup_num_tokens=3, images=1, streamer=1, attention_mask=1)),
        ("inflight: batch state before sharded", lambda: sharded(e, "score", lambda: infl(INFLIGHT, mm_state=batch))),
        ("inflight: sharded", lambda: sharded(e, "score", lambda: infl(INFLIGHT, mm_state=e.mm))),
        ("inflight: engine without slots", lambda: e.model["plain"].generate_inflight(INFLIGHT, mm_state=e.mm)),
        ("inflight: logprobs without the method", lambda: e.model["inflight"].generate_inflight(INFLIGHT, mm_state=e.mm, output_logprobs=True)),
        ("score: batch state before sharded", lambda: sharded(e, "score", lambda: score(PROMPT, CANDIDATES, mm_state=batch))),
        ("score: sharded", lambda: sharded(e, "score", lambda: score(PROMPT, CANDIDATES, mm_state=e.mm))),
        ("score: empty candidate", lambda: score(PROMPT, [[7], []], mm_state=e.mm)),
    ]


def sharded(e, name, thunk):
    e.inner[name].world = 2
    try:
        return thunk()
    finally:
        e.inner[name].world = 1


def case_refusals(e):
    out = []
    for name, thunk in refusals(e):
        try:
            thunk()
            out.append([name, None, None])
        except Exception as ex:      # noqa: BLE001  the type and the text are what is recorded
            out.append([name, type(ex).__name__, str(ex)])
    return out


RAGGED_EOS = 303                                                    # the token row 1 of RAGGED emits second (asserted when the file is written)
CASES = {f.__name__[5:]: f for f in (case_ragged_right_padded_eos, case_sample_two_returns, case_beams, case_left_padded, case_two_videos_row_by_row,
                                     case_prompt_lookup_partly_rejected, case_inflight_logprobs, case_score_two_groups,
                                     case_return_dict_scores_and_hooks, case_refusals)}


def run_case(name):
    """-> {"calls": every engine call of the case, in order, "result": what the entry point returned}"""
    e = env()
    for r in e.rec.values():
        del r.log[:]
    result = plain(CASES[name](e))
    return {"calls": [dict(c, engine=k) for k, r in e.rec.items() for c in r.log], "result": result}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    got = {name: run_case(name) for name in CASES}
    rows = got["ragged_right_padded_eos"]["result"]
    assert rows[1][1] == RAGGED_EOS and rows[1][2:] == [0, 0, 0] and RAGGED_EOS not in rows[0] + rows[2], rows      # one row stops early, alone
    assert all(t is not None for _, t, _ in got["refusals"]["result"]), got["refusals"]["result"]
    assert not got["refusals"]["calls"], "a refused call runs nothing"
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": {\"calls\": [\n  " + ",\n  ".join(json.dumps(c) for c in v["calls"]) + "\n ],\n \"result\": "
                                   + json.dumps(v["result"]) + "}" for k, v in got.items()) + "\n}\n")
    print(out, {k: len(v["calls"]) for k, v in got.items()})
