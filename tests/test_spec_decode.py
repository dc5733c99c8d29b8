"""Prompt-lookup speculative decoding on the CPU: the draft rule against transformers' own class (a committed recording and, when the class
imports, fresh random cases), the accept rule, and `generate(prompt_lookup_num_tokens=...)` over the CPU oracle engine — the tokens of plain
greedy decoding, exactly, whatever the drafts are."""
import json
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from oracle_engine import OracleEngine  # noqa: E402
from util import seeded  # noqa: E402
from vidi_amd.spec import accept_run, lookup_draft  # noqa: E402

CASES = json.load(open(os.path.join(HERE, "golden", "prompt_lookup_cases.json")))["cases"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the draft rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_lookup_draft_reproduces_the_recorded_hf_candidates():
    assert len(CASES) >= 200 and sum(bool(c["draft"]) for c in CASES) >= 50
    names = " | ".join(c["name"] for c in CASES)
    for needed in ("empty continuation", "EOS as first candidate", "history of length 1"):
        assert needed in names
    for c in CASES:
        assert lookup_draft(c["history"], c["num_tokens"], c["max_ngram"], c["eos"]) == c["draft"], c["name"]
    by_name = {c["name"]: c["draft"] for c in CASES}
    assert by_name["no match but the tail itself (empty continuation)"] == [] and by_name["EOS as first candidate"] == []
    assert by_name["history of length 1"] == [] and by_name["EOS in the middle"] == [6]


def test_lookup_draft_against_the_installed_hf_class():
    pytest.importorskip("transformers.generation.candidate_generator")
    from make_prompt_lookup_cases import hf_draft, random_case
    rng = random.Random(77)
    hits = 0
    for _ in range(300):
        c = random_case(rng)
        want = hf_draft(c["history"], c["num_tokens"], c["max_ngram"], c["eos"])
        assert lookup_draft(c["history"], c["num_tokens"], c["max_ngram"], c["eos"]) == want, c
        hits += bool(want)
    assert hits >= 100


def test_lookup_draft_refuses_what_hf_refuses():
    with pytest.raises(ValueError):
        lookup_draft([1, 2, 1], 0, 2, [])
    with pytest.raises(ValueError):
        lookup_draft([1, 2, 1], 3, 0, [])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the accept rule
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argmax,draft,eos,room,want", [
    ([9, 8, 7, 6], [1, 2, 3], [], 10, (0, [9])),                      # none accepted: the model's own token
    ([1, 2, 7, 6], [1, 2, 3], [], 10, (2, [1, 2, 7])),                # some
    ([1, 2, 3, 6], [1, 2, 3], [], 10, (3, [1, 2, 3, 6])),             # all: + the bonus token
    ([1, 5, 3, 6], [1, 5, 3], [5], 10, (3, [1, 5])),                  # EOS inside the accepted run: cut after it
    ([1, 2, 3, 5], [1, 2, 3], [5], 10, (3, [1, 2, 3, 5])),            # EOS as the bonus token
    ([1, 5, 7, 6], [1, 2, 3], [5], 10, (1, [1, 5])),                  # EOS as the model's token at the first disagreement
    ([1, 2, 3, 6], [1, 2, 3], [], 2, (3, [1, 2])),                    # room smaller than the run
    ([1, 2, 3, 6], [1, 2, 3], [], 4, (3, [1, 2, 3, 6])),
    ([4], [], [], 3, (0, [4])),
])
def test_accept_run(argmax, draft, eos, room, want):
    assert accept_run(argmax, draft, eos, room) == want


def test_accept_run_wants_one_row_per_draft_and_one_more():
    with pytest.raises(ValueError):
        accept_run([1, 2], [1, 2], [], 5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. generate() over the oracle engine
# ---------------------------------------------------------------------------------------------------------------------------------------
class SpecOracleEngine(OracleEngine):
    """the oracle engine + what the verify loop needs from an engine: a cache roll-back and the draft limit; records every text_forward"""

    def __init__(self, cfg, w):
        super().__init__(cfg, w)
        self.calls, self.margins, self.last_ts = [], [], None

    def new_text_state(self, B, Lmax):
        self.last_ts = super().new_text_state(B, Lmax)
        return self.last_ts

    def text_forward(self, hidden, positions, ts, mm, Lq, new_mask=None, dyn=False):
        self.calls.append((ts.past_len, Lq))
        return super().text_forward(hidden, positions, ts, mm, Lq, new_mask=new_mask, dyn=dyn)

    def logits_argmax(self, hn_last):
        logits, idx = super().logits_argmax(hn_last)
        top2 = torch.topk(logits.float(), 2, dim=-1).values
        self.margins.extend((top2[:, 0] - top2[:, 1]).tolist())
        return logits, idx

    def truncate_text_state(self, ts, n_keep):
        assert 0 <= n_keep <= ts.past_len
        ts.caches.text = [(k[:, :, :n_keep], v[:, :, :n_keep]) for k, v in ts.caches.text]
        ts.mask = ts.mask[:, :n_keep]
        ts.past_len = n_keep
        ts.n_valid = ts.mask.sum(-1)                                       # the engine owns the count of valid positions

    def spec_max_draft(self):
        return 32 // (self.cfg.num_attention_heads // self.cfg.num_key_value_heads) - 1


N_NEW, K = 13, 3
PROMPT = [2, 21, 22, -200, 23, 24, 25, 21, 22]
# weight seeds, chosen on the CPU: every step of the plain run has a top-2 margin > 1e-3 (asserted in setup()), the 13 tokens vary (one first
# appears inside the second verify step: the EOS case) and lookup drafts occur.  (Vidi1.5 with an untied head: random TIED embeddings echo
# the input token for ever, which would make every draft trivially right.)
SEEDS = {"vidi15": 4, "vidi7b": 2}
_cache = {}


def setup(arch):
    """one model per architecture, its video state and its plain greedy run"""
    if arch not in _cache:
        from types import SimpleNamespace
        from vidi_amd.config import tiny, tiny_7b
        from vidi_amd.model import VidiForCausalLM
        from vidi_amd.weights import init_random_weights
        cfg = tiny(tie_word_embeddings=False) if arch == "vidi15" else tiny_7b()
        w = init_random_weights(cfg, seed=SEEDS[arch], dtype=torch.float32, device="cpu")
        eng = SpecOracleEngine(cfg, w)
        model = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=eng)
        S = cfg.vis_image_size
        mm = model.encode_mm_state(seeded((2, 3, S, S), 702, 0.5).clamp(-1, 1)[None], seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 710, 0.3)[None], [100])
        ids = torch.tensor([PROMPT], dtype=torch.int64)
        run = lambda **kw: model.generate(ids, mm_state=mm, max_new_tokens=N_NEW, eos_token_id=kw.pop("eos", 999999), **kw)[0].tolist()   # noqa: E731
        eng.margins = []
        plain = run()
        assert len(plain) == N_NEW and min(eng.margins) > 1e-3, (arch, min(eng.margins))
        _cache[arch] = SimpleNamespace(cfg=cfg, eng=eng, model=model, run=run, plain=plain, plain_len=eng.last_ts.past_len, n_prompt=len(PROMPT) - 1)
    s = _cache[arch]
    s.eng.calls = []
    s.model.__dict__.pop("_spec_draft", None)
    return s


def forced(s, wrong_at=()):
    """a draft function that proposes the plain run's continuation; positions (within a draft) listed in `wrong_at` hold another token"""
    def draft(history, k, max_ngram, eos_ids):
        n_new = len(history) - s.n_prompt
        assert history[s.n_prompt:] == s.plain[:n_new]
        d = s.plain[n_new: n_new + k]
        return [(t + 1) % s.cfg.vocab_size if i in wrong_at else t for i, t in enumerate(d)]
    return draft


ARCHS = ["vidi15", "vidi7b"]


@pytest.mark.parametrize("arch", ARCHS)
def test_generate_with_lookup_drafts_equals_plain_greedy(arch):
    s = setup(arch)
    assert s.run(prompt_lookup_num_tokens=K) == s.plain
    assert s.eng.calls[0] == (0, len(PROMPT) - 1) and max(lq for _, lq in s.eng.calls[1:]) > 1, "no lookup draft was verified: pick another seed"
    assert s.run(prompt_lookup_num_tokens=K, max_matching_ngram_size=1) == s.plain


@pytest.mark.parametrize("arch", ARCHS)
def test_generate_with_oracle_drafts_takes_three_verify_steps(arch):
    s = setup(arch)
    s.model._spec_draft = forced(s)
    assert s.run(prompt_lookup_num_tokens=K) == s.plain
    L = len(PROMPT) - 1
    assert s.eng.calls == [(0, L), (L, 4), (L + 4, 4), (L + 8, 4)]             # one prefill + 3 verify steps of K + 1 rows: 1 + 3 * 4 = 13 tokens


@pytest.mark.parametrize("arch", ARCHS)
def test_generate_with_wrong_drafts_rolls_the_cache_back(arch):
    s = setup(arch)
    s.model._spec_draft = forced(s, wrong_at=(0, 1, 2))
    assert s.run(prompt_lookup_num_tokens=K) == s.plain
    ts = s.eng.last_ts
    assert ts.past_len == s.plain_len == ts.mask.shape[1] == ts.caches.text[0][0].shape[2]
    assert int(ts.n_valid[0]) == s.plain_len
    assert [lq for _, lq in s.eng.calls[1:]] == [4] * 9 + [3, 2, 1]            # every step yields one token; the draft shrinks with the room left


@pytest.mark.parametrize("arch", ARCHS)
def test_generate_with_two_right_drafts_and_a_wrong_third(arch):
    s = setup(arch)
    s.model._spec_draft = forced(s, wrong_at=(2,))
    assert s.run(prompt_lookup_num_tokens=K) == s.plain
    L = len(PROMPT) - 1
    assert s.eng.calls[1:4] == [(L, 4), (L + 3, 4), (L + 6, 4)]               # two drafts + the model's own token per step
    assert s.eng.last_ts.past_len == s.plain_len


@pytest.mark.parametrize("arch", ARCHS)
def test_generate_stops_at_an_eos_inside_an_accepted_run(arch):
    s = setup(arch)
    at = next(i for i in range(5, N_NEW) if s.plain[i] not in s.plain[:i])     # a token whose first appearance lies inside the second verify step
    assert 5 <= at <= 7, (at, s.plain)
    eos = s.plain[at]
    want = s.run(eos=eos)
    assert want == s.plain[: at + 1]
    s.model._spec_draft = forced(s)
    assert s.run(prompt_lookup_num_tokens=K, eos=eos) == want
    assert s.run(prompt_lookup_num_tokens=K, eos=[999999, eos]) == want


def test_streamer_receives_the_tokens_in_order():
    s = setup("vidi15")

    class Streamer:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got.extend(t.reshape(-1).tolist())

        def end(self):
            self.ended = True
    st = Streamer()
    s.model._spec_draft = forced(s, wrong_at=(1,))
    assert s.run(prompt_lookup_num_tokens=K, streamer=st) == s.plain
    assert st.got == s.plain and st.ended


def test_a_request_beyond_the_draft_limit_is_clipped():
    s = setup("vidi15")
    s.model._spec_draft = forced(s)
    assert s.run(prompt_lookup_num_tokens=100) == s.plain
    assert s.eng.spec_max_draft() == 15 and max(lq for _, lq in s.eng.calls[1:]) == 12     # room - 1 = 11 drafts after the first token


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. what is refused
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    s = setup("vidi15")
    ids = torch.tensor([PROMPT], dtype=torch.int64)
    gen = lambda i=ids, **kw: s.model.generate(i, max_new_tokens=3, prompt_lookup_num_tokens=4, **kw)      # noqa: E731
    assert gen().shape == (1, 3)                                          # the supported case no longer raises
    with pytest.raises(ValueError):
        gen(ids.repeat(2, 1))
    with pytest.raises(ValueError):
        s.model.generate(ids, max_new_tokens=3, prompt_lookup_num_tokens=-1)
    for kw in (dict(do_sample=True), dict(num_beams=2), dict(logits_processor=[lambda i, x: x]), dict(repetition_penalty=1.3),
               dict(no_repeat_ngram_size=2), dict(stopping_criteria=[lambda i, x: False]), dict(max_time=5.0), dict(return_dict_in_generate=True)):
        with pytest.raises(NotImplementedError):
            gen(**kw)
    from vidi_amd.engine import MMBatchState
    with pytest.raises(NotImplementedError):
        gen(mm_state=MMBatchState.__new__(MMBatchState))
    s.eng.world = 2
    try:
        with pytest.raises(NotImplementedError):
            gen()
    finally:
        s.eng.world = 1
    from vidi_amd.model import VidiForCausalLM
    plain_eng = OracleEngine(s.cfg, s.eng.w)                              # an engine that cannot roll its cache back
    m2 = VidiForCausalLM(s.cfg, s.eng.w, dtype=torch.float32, device="cpu", engine=plain_eng)
    with pytest.raises(NotImplementedError):
        m2.generate(ids, max_new_tokens=3, prompt_lookup_num_tokens=4)
    assert m2.generate(ids, max_new_tokens=3).shape == (1, 3)
